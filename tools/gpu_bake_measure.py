"""GPU: first measurements of the baked probe tables (profiles/bake.txt).

A. Probes per second of PvAmdBakeRun with one solver and with two on one GPU, against PvAmdRunAsync runs alone at the same
   listeners (the same dealing: round-robin, one run in flight per solver): SmallRoomScene.pv at 275 Hz (25 m, the resident
   kernel) and HugeRoom.pv in a 2048^2 grid (Mode A, 275 Hz).
B. Stored bytes per probe (records and file).
C. PvAmdBakeQueryDevice for 10^6 queries (upload cached; transfers included) and PvAmdBakeQuery on the host.
D. For information: interpolation error per field at 64 off-lattice listeners against their simulated PvAmdGetOutput.

    python tools/gpu_bake_measure.py [out.json]          all of it
    python tools/gpu_bake_measure.py --trace             one short bake per workload (for rocprofv3 --kernel-trace --stats)
"""
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from planeverb_amd import api  # noqa: E402

DX = np.float32(343.21) / np.float32(275) / np.float32(3.5)
SCENES = os.path.join(ROOT, "tests", "scenes")
NAMES = ["occlusion", "wetGain", "rt60", "lowpass", "directionX", "directionY", "sourceDirectionX", "sourceDirectionY"]


def workloads():
    n = 2048
    size = float((n + 0.5) * DX)
    return [
        dict(name="SmallRoomScene 25 m @ 275 Hz", size=25.0, scene="SmallRoomScene.pv", lattice=(2, 1.0, 1.0, 1.0, 1.0, 23, 23)),
        dict(name="HugeRoom.pv 2048^2 Mode A", size=size, scene="HugeRoom.pv",
             lattice=(8, size * 0.2, size * 0.2, size * 0.1, size * 0.1, 7, 7)),
    ]


def solvers(w, n):
    out = []
    for i in range(n):
        s = api.Solver(w["size"], w["size"], 275, **({"stream_priority": 1} if i else {}))
        s.load_scene(os.path.join(SCENES, w["scene"]))
        out.append(s)
    return out


def runs_only(ss, listeners):
    t = time.perf_counter()
    for q, L in enumerate(listeners):
        ss[q % len(ss)].run_async(L)
    for s in ss:
        s.sync()
    return time.perf_counter() - t


def measure(w, reps=2):
    r = dict(workload=w["name"])
    for n in (1, 2):
        ss = solvers(w, n)
        b = api.Bake(ss[0], *w["lattice"])
        b.run(ss)  # warm-up (graph capture, resident claims) and the probe states
        info = b.info()
        valid = [k for k in range(info["nx"] * info["nz"]) if b.probe(k)[0][0] == 1]
        L = [(float(np.float32(info["x0"]) + np.float32(k % info["nx"]) * np.float32(info["sx"])), 0.0,
              float(np.float32(info["z0"]) + np.float32(k // info["nx"]) * np.float32(info["sz"]))) for k in valid]
        tb, tr = [], []
        for _ in range(reps):
            tr.append(runs_only(ss, L))
            t = time.perf_counter()
            b.run(ss)
            tb.append(time.perf_counter() - t)
        r["solvers%d" % n] = dict(probes=len(valid), bake_probes_per_s=len(valid) / min(tb), runs_per_s=len(valid) / min(tr),
                                  ratio=min(tr) / min(tb))
        if n == 1:
            with tempfile.TemporaryDirectory() as d:
                p = os.path.join(d, "b.pvbake")
                b.save(p)
                fb = os.path.getsize(p)
            r["bytes_per_probe_records"] = info["records"] * 36 / max(info["probesBaked"], 1)
            r["bytes_per_probe_file"] = fb / max(info["probesBaked"], 1)
            r["probes_invalid"] = info["probesInvalid"]
            r["stride"] = info["stride"]
            keep = (b, ss)
        else:
            for s in ss:
                s.close()
    b, ss = keep
    # C. queries
    rng = np.random.default_rng(1)
    nq = 1_000_000
    Lq = np.zeros((nq, 3), np.float32)
    Eq = np.zeros((nq, 3), np.float32)
    Lq[:, 0], Lq[:, 2] = rng.uniform(0, w["size"], nq), rng.uniform(0, w["size"], nq)
    Eq[:, 0], Eq[:, 2] = rng.uniform(0, w["size"], nq), rng.uniform(0, w["size"], nq)
    b.query_device(Lq[:1000], Eq[:1000], 0)  # upload
    t = time.perf_counter()
    dev = b.query_device(Lq, Eq, 0)
    r["device_queries_per_s"] = nq / (time.perf_counter() - t)
    t = time.perf_counter()
    host = b.query(Lq[:100_000], Eq[:100_000])
    r["host_queries_per_s"] = 100_000 / (time.perf_counter() - t)
    r["device_equals_host_100k"] = bool(np.array_equal(dev[:100_000].view(np.uint32), host.view(np.uint32)))
    # D. interpolation error at 64 off-lattice listeners (air cells), 16 emitters each
    beta, _ = ss[0].material()
    s = ss[0]
    errs = {k: [] for k in NAMES}
    got_n = 0
    while got_n < 64:
        L = (float(rng.uniform(0.05, 0.95) * w["size"]), 0.0, float(rng.uniform(0.05, 0.95) * w["size"]))
        cx, cy = int(np.float32(L[0]) / DX), int(np.float32(L[2]) / DX)
        if beta[cx, cy] == 0:
            continue
        got_n += 1
        s.run(L)
        E = np.stack([rng.uniform(0, w["size"], 16), np.zeros(16), rng.uniform(0, w["size"], 16)], 1).astype(np.float32)
        q = b.query(np.repeat(np.array([L], np.float32), 16, 0), E)
        for e, qq in zip(E, q):
            o = s.get_output(tuple(float(v) for v in e)).as_array()
            if qq[0] == -1 or o[0] == -1 or o[0] == 0:
                continue
            for m, k in enumerate(NAMES):
                if np.isfinite(qq[m]) and np.isfinite(o[m]):
                    errs[k].append(abs(float(qq[m]) - float(o[m])))
    r["interp_abs_err_median_p90"] = {k: [float(np.median(v)), float(np.percentile(v, 90)), len(v)] if v else None
                                      for k, v in errs.items()}
    for s in ss:
        s.close()
    b.close()
    return r


def main():
    if "--trace" in sys.argv:
        for w in workloads():
            ss = solvers(w, 1)
            b = api.Bake(ss[0], *w["lattice"])
            b.run(ss)
            print("%s: %d probes baked" % (w["name"], b.info()["probesBaked"]))
            b.close()
            ss[0].close()
        return
    out = [measure(w) for w in workloads()]
    txt = json.dumps(out, indent=1)
    print(txt)
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    if args:
        with open(args[0], "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
