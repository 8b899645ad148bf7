"""numpy restatement of the baked probe tables of INTEGRATION.md ("Baked probe tables"): the query rule and a writer of the file
format, written from that document (not from csrc/pv_bake.*).  float32 throughout; every product and sum is its own rounding."""
import struct

import numpy as np

f32 = np.float32
FLT_MAX = np.finfo(np.float32).max
MAGIC = b"PVBAKE\x00\x01"
VERSION = 1
HEADER = struct.Struct("<8sI5ifi4f2i2iqQ")  # 88 bytes
ENTRY = struct.Struct("<5iQ")               # 28 bytes


def fnv1a64(data, h=14695981039346656037):
    for b in data:
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


class RefBake:
    """hdr: dict gx gy T fs res dx stride x0 z0 sx sz nx nz materialHash; probes: list of nx*nz (state, i0, j0, ni, nj, rec) with
    rec float32 [ni, nj, 9]"""

    def __init__(self, hdr, probes):
        self.h = dict(hdr)
        self.probes = probes

    def counts(self):
        st = [p[0] for p in self.probes]
        return sum(s != 0 for s in st), sum(s == 2 for s in st), sum(int(p[3]) * int(p[4]) for p in self.probes)

    def to_bytes(self):
        h = self.h
        baked, invalid, records = self.counts()
        out = [HEADER.pack(MAGIC, VERSION, h["gx"], h["gy"], h["T"], h["fs"], h["res"], f32(h["dx"]), h["stride"], f32(h["x0"]),
                           f32(h["z0"]), f32(h["sx"]), f32(h["sz"]), h["nx"], h["nz"], baked, invalid, records, h["materialHash"])]
        off = HEADER.size + ENTRY.size * len(self.probes)
        for st, i0, j0, ni, nj, rec in self.probes:
            out.append(ENTRY.pack(st, i0, j0, ni, nj, off))
            off += 36 * ni * nj
        for p in self.probes:
            out.append(np.ascontiguousarray(p[5], "<f4").tobytes())
        body = b"".join(out)
        return body + struct.pack("<Q", fnv1a64(body))

    def write(self, path):
        with open(path, "wb") as f:
            f.write(self.to_bytes())

    def query(self, L, E):
        """L, E: [n, 3] float32 listener / emitter positions -> [n, 8] float32"""
        h = self.h
        L = np.asarray(L, f32).reshape(-1, 3)
        E = np.asarray(E, f32).reshape(-1, 3)
        n = len(L)
        gx, gy, d, nx, nz = h["gx"], h["gy"], h["stride"], h["nx"], h["nz"]
        dx, x0, z0, sx, sz = f32(h["dx"]), f32(h["x0"]), f32(h["z0"]), f32(h["sx"]), f32(h["sz"])
        P = self.probes
        state = np.array([p[0] for p in P], np.int64)
        pi0 = np.array([p[1] for p in P], np.int64)
        pj0 = np.array([p[2] for p in P], np.int64)
        pni = np.array([p[3] for p in P], np.int64)
        pnj = np.array([p[4] for p in P], np.int64)
        sizes = pni * pnj * 9
        off = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
        rec = np.concatenate([np.asarray(p[5], f32).reshape(-1) for p in P] + [np.zeros(9, f32)])
        with np.errstate(all="ignore"):
            # 1. emitter cell
            qr = (E[:, 0] + f32(0)) / dx
            qc = (E[:, 2] + f32(0)) / dx
            valid = (qr > f32(-1)) & (qr < f32(gx)) & (qc > f32(-1)) & (qc < f32(gy))
            er = np.where(valid, qr, f32(0)).astype(np.int64)  # truncation toward zero
            ec = np.where(valid, qc, f32(0)).astype(np.int64)
            # 2. emitter corners
            ei0, ej0 = er // d, ec // d
            fa = (er - ei0 * d).astype(f32) / f32(d)
            fb = (ec - ej0 * d).astype(f32) / f32(d)
            # 3. probe corners
            p = (L[:, 0] - x0) / sx
            q = (L[:, 2] - z0) / sz
            p = np.where(p >= f32(0), p, f32(0))
            q = np.where(q >= f32(0), q, f32(0))
            p = np.where(p <= f32(nx - 1), p, f32(nx - 1)).astype(f32)
            q = np.where(q <= f32(nz - 1), q, f32(nz - 1)).astype(f32)
            k0 = np.zeros(n, np.int64) if nx == 1 else np.minimum(np.floor(p).astype(np.int64), nx - 2)
            m0 = np.zeros(n, np.int64) if nz == 1 else np.minimum(np.floor(q).astype(np.int64), nz - 2)
            fp = p - k0.astype(f32)
            fq = q - m0.astype(f32)
            one = f32(1)
            # 4. contributions
            used = np.zeros(n, np.int64)
            first = np.zeros((n, 9), f32)
            S = np.zeros(n, f32)
            acc = np.zeros((n, 8), f32)
            den = np.zeros(n, f32)
            any_inf = np.zeros(n, bool)
            for pc in range(4):
                a, b = pc & 1, pc >> 1
                pi, pj = k0 + a, m0 + b
                wp = (fp if a else one - fp) * (fq if b else one - fq)
                inr = (pi < nx) & (pj < nz)
                k = np.where(inr, pj * nx + pi, 0)
                ok = inr & (state[k] == 1) & valid
                for ecn in range(4):
                    ea, eb = ecn & 1, ecn >> 1
                    we = (fa if ea else one - fa) * (fb if eb else one - fb)
                    w = (wp * we).astype(f32)
                    ni = ei0 + ea - pi0[k]
                    nj = ej0 + eb - pj0[k]
                    inb = ok & (w > 0) & (ni >= 0) & (ni < pni[k]) & (nj >= 0) & (nj < pnj[k])
                    idx = np.where(inb, off[k] + (ni * pnj[k] + nj) * 9, len(rec) - 9)
                    r = rec[idx[:, None] + np.arange(9)]
                    use = inb & (r[:, 8] < FLT_MAX)
                    first = np.where((use & (used == 0))[:, None], r, first)
                    used += use
                    S = np.where(use, S + w, S)
                    for m in (0, 1, 3, 4, 5, 6, 7):
                        acc[:, m] = np.where(use, acc[:, m] + w * r[:, m], acc[:, m])
                    fin = use & np.isfinite(r[:, 2])
                    acc[:, 2] = np.where(fin, acc[:, 2] + w * r[:, 2], acc[:, 2])
                    den = np.where(fin, den + w, den)
                    any_inf |= use & (r[:, 2] == np.inf)
            # 5. result
            out = np.zeros((n, 8), f32)
            for m in (0, 1, 3):
                out[:, m] = acc[:, m] / S
            out[:, 2] = np.where(den > 0, acc[:, 2] / den, np.where(any_inf, f32(np.inf), f32(np.nan)))
            for m in (4, 6):
                x, y = acc[:, m], acc[:, m + 1]
                ln = x * x + y * y
                nz_ = ln != 0
                s = np.sqrt(np.where(nz_, ln, f32(1)))
                out[:, m] = np.where(nz_, x / s, f32(0))
                out[:, m + 1] = np.where(nz_, y / s, f32(0))
            out = np.where((used == 1)[:, None], first[:, :8], out)
            sentinel = np.zeros(8, f32)
            sentinel[0] = -1
            out = np.where((used == 0)[:, None], sentinel, out)
        return out.astype(f32)


def random_bake(rng, gx=37, gy=29, stride=3, nx=4, nz=3, dx=0.25, x0=0.5, z0=0.75, sx=1.25, sz=1.5, p_state=(0.15, 0.7, 0.15),
                p_empty=0.1, p_reached=0.75):
    """a bake of random contents over the whole state space: states 0 / 1 / 2, empty blocks, unreached nodes, rt60 finite / NaN / +inf"""
    li, lj = -(-gx // stride), -(-gy // stride)
    hdr = dict(gx=gx, gy=gy, T=435, fs=1443, res=275, dx=f32(dx), stride=stride, x0=f32(x0), z0=f32(z0), sx=f32(sx), sz=f32(sz),
               nx=nx, nz=nz, materialHash=int(rng.integers(0, 2**63)))
    probes = []
    for _ in range(nx * nz):
        st = int(rng.choice(3, p=p_state))
        if st != 1 or rng.random() < p_empty:
            probes.append((st, 0, 0, 0, 0, np.zeros((0, 0, 9), f32)))
            continue
        ni, nj = int(rng.integers(1, li + 1)), int(rng.integers(1, lj + 1))
        i0, j0 = int(rng.integers(0, li - ni + 1)), int(rng.integers(0, lj - nj + 1))
        rec = rng.uniform(-1, 1, (ni, nj, 9)).astype(f32)
        rec[..., 0] = rng.uniform(0, 1.2, (ni, nj))
        rt = rng.uniform(0.05, 3, (ni, nj)).astype(f32)
        kind = rng.random((ni, nj))
        rt[kind < 0.15] = np.nan
        rt[(kind >= 0.15) & (kind < 0.3)] = np.inf
        rec[..., 2] = rt
        reached = rng.random((ni, nj)) < p_reached
        rec[..., 8] = np.where(reached, rng.integers(0, 430, (ni, nj)).astype(f32), FLT_MAX)
        rec[~reached, :8] = 0
        probes.append((st, i0, j0, ni, nj, rec))
    return RefBake(hdr, probes)


def random_pairs(rng, h, n):
    """listeners around the probe lattice (outside it too), emitters around the grid (outside it too), some on exact nodes"""
    nx, nz, sx, sz = h["nx"], h["nz"], float(h["sx"]), float(h["sz"])
    L = np.zeros((n, 3), f32)
    L[:, 0] = rng.uniform(float(h["x0"]) - 2 * sx, float(h["x0"]) + (nx + 1) * sx, n)
    L[:, 2] = rng.uniform(float(h["z0"]) - 2 * sz, float(h["z0"]) + (nz + 1) * sz, n)
    dx = float(h["dx"])
    E = np.zeros((n, 3), f32)
    E[:, 0] = rng.uniform(-3 * dx, (h["gx"] + 3) * dx, n)
    E[:, 2] = rng.uniform(-3 * dx, (h["gy"] + 3) * dx, n)
    m = n // 4  # exact probe positions and emitter nodes
    L[:m, 0] = f32(h["x0"]) + rng.integers(0, nx, m).astype(f32) * f32(sx)
    L[:m, 2] = f32(h["z0"]) + rng.integers(0, nz, m).astype(f32) * f32(sz)
    d = h["stride"]
    E[:m, 0] = ((rng.integers(0, -(-h["gx"] // d), m) * d).astype(f32) + f32(0.5)) * f32(dx)
    E[:m, 2] = ((rng.integers(0, -(-h["gy"] // d), m) * d).astype(f32) + f32(0.5)) * f32(dx)
    return L, E
