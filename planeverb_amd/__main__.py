"""Headless command line for the solver: load a .pv scene, simulate one listener position,
print the acoustic parameters of each emitter as JSON -- the numbers the Sandbox shows in its "Analyzer Output" panel
(PlaneverbSandbox/src/Editor/Editor.cpp:396-434) without the GUI.

    python -m planeverb_amd tests/scenes/SmallRoomScene.pv --listener 5,0,4 --emitter 5,0,6 --emitter 12,0,9
    python -m planeverb_amd tests/scenes/HugeRoom.pv --cells 4096 --listener 5,0,4 --emitter 5,0,6
    python -m planeverb_amd scene.pv --save copy.pv          # .pv round trip (Editor::SaveGeometry format)
"""
import argparse
import json
import sys

import numpy as np

from . import api


def vec3(s):
    v = [float(x) for x in s.split(",")]
    if len(v) != 3:
        raise argparse.ArgumentTypeError("expected x,y,z")
    return tuple(v)


def echogram_setting(s):
    v = s.split(",")
    if len(v) != 2:
        raise argparse.ArgumentTypeError("expected slotSeconds,nSlots")
    return float(v[0]), int(v[1])


def waterfall_bins(s):
    v = s.split(",")
    if len(v) != 3 or int(v[2]) < 1:
        raise argparse.ArgumentTypeError("expected F0,F1,N")
    return np.linspace(float(v[0]), float(v[1]), int(v[2])).astype(np.float32)


def array_members(s):
    """one array: x,z,gain,delay;x,z,gain,delay;... -> [((x, 0, z), gain, delaySeconds)]"""
    out = []
    for part in s.split(";"):
        v = [float(x) for x in part.split(",")]
        if len(v) != 4:
            raise argparse.ArgumentTypeError("expected x,z,gain,delay;x,z,gain,delay;...")
        out.append(((v[0], 0.0, v[1]), v[2], v[3]))
    return out


def echogram_window(s):
    v = s.split(",")
    if len(v) != 2:
        raise argparse.ArgumentTypeError("expected zeroCrossings,beta")
    return int(v[0]), float(v[1])


def read_signal(path, rate):
    """a dry mono signal as float32 [N]: a 1-D .npy, or a 16-bit PCM mono .wav whose rate is `rate` (samples / 32768)"""
    if path.lower().endswith(".wav"):
        import wave
        with wave.open(path, "rb") as f:
            if f.getnchannels() != 1 or f.getsampwidth() != 2 or f.getcomptype() != "NONE":
                raise ValueError("%s: expected 16-bit PCM mono" % path)
            if f.getframerate() != rate:
                raise ValueError("%s: its rate is %d, --aural-rate is %d" % (path, f.getframerate(), rate))
            x = np.frombuffer(f.readframes(f.getnframes()), "<i2").astype(np.float32) / np.float32(32768.0)
    else:
        x = np.load(path)
        if x.ndim != 1:
            raise ValueError("%s: expected a 1-D array" % path)
        x = x.astype(np.float32)
    if not 1 <= x.size <= api.AURAL_MAX_SAMPLES:
        raise ValueError("%s: 1 .. %d samples" % (path, api.AURAL_MAX_SAMPLES))
    return np.ascontiguousarray(x)


def write_signal(path, x, rate):
    """float32 .npy as it is, or a 16-bit PCM mono .wav normalised to its peak (silence and non-finite samples: zeros)"""
    if path.lower().endswith(".wav"):
        import wave
        y = np.where(np.isfinite(x), x, np.float32(0.0)).astype(np.float64)
        peak = np.abs(y).max() if y.size else 0.0
        pcm = np.round(y / peak * 32767.0).astype("<i2") if peak > 0 else np.zeros(y.size, "<i2")
        with wave.open(path, "wb") as f:
            f.setnchannels(1)
            f.setsampwidth(2)
            f.setframerate(rate)
            f.writeframes(pcm.tobytes())
    else:
        with open(path, "wb") as f:  # (np.save would append .npy to another suffix)
            np.save(f, np.ascontiguousarray(x, np.float32))


def rect4(s):
    v = [float(x) for x in s.split(",")]
    if len(v) != 4:
        raise argparse.ArgumentTypeError("expected xmin,zmin,xmax,zmax")
    return tuple(v)


def zone_plane_names(s, a):
    """(kind name, JSON key, the names of its planes) of every map the options asked for, in the maps' plane order"""
    kinds = []
    if a.room_metrics:
        kinds.append(("room_metrics", "roomMetrics", list(api.ROOM_METRIC_NAMES)))
    if a.decay_times:
        kinds.append(("decay_times", "decayTimes", list(api.DECAY_TIME_NAMES)))
    if a.lateral_fraction:
        kinds.append(("lateral_fraction", "lateralFraction", list(api.LATERAL_FRACTION_NAMES)))
    if a.echo_criterion:
        kinds.append(("echo_criterion", "echoCriterion", list(api.ECHO_CRITERION_NAMES)))
    if a.echogram:
        kinds.append(("echogram", "echogram", ["n"] + ["%s[%d]" % (n, j) for j in range(s.echogram_slots()[0]) for n in ("e", "ix", "iy")]))
    if a.lobes is not None:
        kinds.append(("lobes", "lobes", ["n"] + ["%s[%d]" % (n, w) for w in range(len(s.lobe_windows()[0]) + 1) for n in api.LOBE_NAMES]))
    if a.bands:
        kinds.append(("band_metrics", "bandMetrics", ["%gHz.%s" % (hz, n) for hz in a.bands for n in api.BAND_METRIC_NAMES]))
    if a.modulation:
        kinds.append(("modulation", "modulation", ["%gHz.%s" % (hz, n) for hz in a.bands
                                                   for n in ["m[%d]" % j for j in range(api.MODULATION_FREQS)] + ["mti"]]))
    if a.spectrum:
        kinds.append(("spectrum", "spectrum", ["%gHz.%s" % (hz, n) for hz in a.spectrum for n in ("re", "im", "levelDb")]))
    return kinds


def zone_tables(s, a):
    """one table per --zone: for every plane of every computed map its n (finite members), mean, std, min and max over the zone"""
    labels = api.zone_labels_from_rects(s.dx, s.gx, s.gy, a.zone)
    if not a.sparse_emitters:  # (there the labels were set in front of the run, which accumulated the curves and the zone maps)
        s.set_zones(labels, len(a.zone))
    tables = [{"rect": list(r), "cells": int((labels == j + 1).sum())} for j, r in enumerate(a.zone)]
    # (sparse-emitter mode: the two kinds a run can accumulate -- Solver.set_zone_maps --, the same tables from the run's own maps)
    streamed = ("room_metrics", "spectrum")
    for kind, key, names in [k for k in zone_plane_names(s, a) if not a.sparse_emitters or k[0] in streamed]:
        recs = s.zone_stats(kind).reshape(len(a.zone), -1)
        for t, row in zip(tables, recs):
            t[key] = dict((n, {"n": int(r["n_finite"]), "mean": float(r["mean"]), "std": float(r["std"]), "min": float(r["min"]),
                               "max": float(r["max"])}) for n, r in zip(names, row))
    if a.zone_decay:
        recs, etc, edc = s.zone_decay(a.zone_decay, curves=True)
        for t, r, e, d in zip(tables, recs, etc, edc):
            t["zoneDecay"] = {"align": a.zone_decay, "nCells": int(r["n_cells"]), "tFirst": int(r["t_first"]), "tLast": int(r["t_last"]),
                              "edt": float(r["edt"]), "t20": float(r["t20"]), "t30": float(r["t30"]), "depth": float(r["depth"]),
                              "nEdt": int(r["n_edt"]), "nT20": int(r["n_t20"]), "nT30": int(r["n_t30"])}
            if a.zone_decay_curves:
                t["zoneDecay"]["etc"] = [float(v) for v in e]
                t["zoneDecay"]["edc"] = [float(v) for v in d]
    if a.zone_band_decay:
        recs, etc, edc = s.zone_band_decay(a.zone_decay, curves=True)
        for t, rz, ez, dz in zip(tables, recs, etc, edc):
            t["zoneBandDecay"] = []
            for hz, r, e, d in zip(a.bands, rz, ez, dz):
                b = {"hz": hz, "align": a.zone_decay, "edt": float(r["edt"]), "t20": float(r["t20"]), "t30": float(r["t30"]),
                     "depth": float(r["depth"]), "nEdt": int(r["n_edt"]), "nT20": int(r["n_t20"]), "nT30": int(r["n_t30"]),
                     "c50": float(r["c50"]), "c80": float(r["c80"]), "d50": float(r["d50"]), "ts": float(r["ts"])}
                if a.zone_decay_curves:
                    b["etc"] = [float(v) for v in e]
                    b["edc"] = [float(v) for v in d]
                t["zoneBandDecay"].append(b)
    return tables


def record_object(kind, m, slot_steps=0):
    """the JSON object of one record (the key names of RECORD_KEYS)"""
    if kind == api.QREC_ECHOGRAM:
        return {"slotSteps": slot_steps, "n": float(m[0]), "e": [float(v) for v in m[1::3]], "ix": [float(v) for v in m[2::3]],
                "iy": [float(v) for v in m[3::3]]}
    if kind == api.QREC_LOBES:
        return {"n": float(m[0]), "windows": [dict((n, float(v)) for n, v in zip(api.LOBE_NAMES, m[1 + 5 * w:6 + 5 * w]))
                                              for w in range((len(m) - 1) // 5)]}
    names = {api.QREC_ROOM_METRICS: api.ROOM_METRIC_NAMES, api.QREC_DECAY_TIMES: api.DECAY_TIME_NAMES,
             api.QREC_LATERAL: api.LATERAL_FRACTION_NAMES, api.QREC_ECHO_CRITERION: api.ECHO_CRITERION_NAMES}[kind]
    return dict((n, float(v)) for n, v in zip(names, m))


RECORD_KEYS = {api.QREC_ROOM_METRICS: "roomMetrics", api.QREC_DECAY_TIMES: "decayTimes", api.QREC_LATERAL: "lateralFraction",
               api.QREC_ECHOGRAM: "echogram", api.QREC_ECHO_CRITERION: "echoCriterion", api.QREC_LOBES: "lobes"}


def live_emission_records(size, res, boxes, listener, emitters, echogram, lobes, slot_steps):
    """all six record kinds of each emitter from the LIVE module (PlaneverbSetEmissionRecords / PlaneverbGetEmissionRecord): the
    scene and the emitters go in as a game would put them, three iterations later the records are read by emission id"""
    api.Init(api.Config((size, size), res, 0, ".", 0, api.pv_GPU))
    try:
        api.SetListenerPosition(listener)
        for b in boxes:
            api.AddGeometry(b)
        ids = [api.Emit(e) for e in emitters]
        api.SetEmissionEchogram(*echogram)
        api.SetEmissionLobeWindows(lobes)
        api.SetEmissionRecords(api.QREC_ALL)
        target = api.IterationCount() + 3
        if api.WaitIterations(target, 120000) < target or api.EmissionRecordKinds() != api.QREC_ALL:
            raise api.PlaneverbError("the live module did not publish the emission records: " + api.last_error())
        return [dict((RECORD_KEYS[k], record_object(k, api.GetEmissionRecord(i, k)[1], slot_steps)) for k in RECORD_KEYS) for i in ids]
    finally:
        api.Exit()


def mesh_setting(v):
    """FILE.npz[,absorption[,shell:r]] -> (path, absorption, mode, radius)"""
    parts = v.split(",")
    try:
        absorption = float(parts[1]) if len(parts) > 1 else 0.5
        mode, radius = api.MESH_SOLID, 0.0
        if len(parts) > 2:
            if not parts[2].startswith("shell:") or len(parts) > 3:
                raise ValueError
            mode, radius = api.MESH_SHELL, float(parts[2][6:])
    except ValueError:
        raise argparse.ArgumentTypeError("expected FILE.npz[,absorption[,shell:r]]")
    return parts[0], absorption, mode, radius


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m planeverb_amd", description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("scene", help=".pv scene file")
    ap.add_argument("--size", type=float, default=25.0, help="grid size in metres (square), default 25 (Sandbox)")
    ap.add_argument("--cells", type=int, default=0, help="instead of --size: N cells per side at --res (Mode A)")
    ap.add_argument("--res", type=int, default=275, help="grid resolution in Hz (>= 275)")
    ap.add_argument("--listener", type=vec3, default=(5.0, 0.0, 4.0))
    ap.add_argument("--emitter", type=vec3, action="append", default=[])
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--room-metrics", action="store_true",
                    help="add the room metrics (C50, C80, D50, Ts and their sums) of each emitter's cell")
    ap.add_argument("--decay-times", action="store_true",
                    help="add the decay times (EDT, T20, T30, their point counts, E0 and the curve's depth) of each emitter's cell")
    ap.add_argument("--lateral-fraction", action="store_true",
                    help="add the early lateral energy fraction, the early-sound direction and their sums of each emitter's cell")
    ap.add_argument("--echogram", metavar="SECONDS,SLOTS", type=echogram_setting,
                    help="add the directional echogram of each emitter's cell: energy and flux (ix, iy: the direction the sound "
                         "travels in) per time slot after the onset, e.g. 0.005,16")
    ap.add_argument("--echo-criterion", action="store_true",
                    help="add the echo criterion (Dietsch and Kraak: EK, its delay, the late EK, its delay and Ts, for speech "
                         "and for music) of each emitter's cell")
    ap.add_argument("--lobes", metavar="SECONDS[,SECONDS...]", nargs="?", const=[], default=None,
                    type=lambda v: [float(x) for x in v.split(",")],
                    help="add the directional energy lobes of each emitter's cell: per time window after the onset the energy and "
                         "its split over the travel directions +x, -x, +y, -y; the window edges in seconds, e.g. 0.005,0.02,0.08 "
                         "(bare flag: 0.01,0.08)")
    ap.add_argument("--spectrum", metavar="HZ[,HZ...]", type=lambda v: [float(x) for x in v.split(",")],
                    help="add the transfer function (re, im, level in dB re the source) of each emitter's cell at these frequencies")
    ap.add_argument("--waterfall", metavar="F0,F1,N", type=waterfall_bins,
                    help="add the waterfall (cumulative spectral decay) of each emitter's cell at the N bins np.linspace(F0, F1, N): "
                         "the complex response of the whole decay and the level in dB re the source of every slice of "
                         "--waterfall-slices; works with and without --sparse-emitters (at most %d emitters)" % api.WATERFALL_MAX_RECEIVERS)
    ap.add_argument("--waterfall-slices", metavar="SEC,M", type=echogram_setting, default=(0.02, 16),
                    help="with --waterfall: M slices, slice k starting k * SEC seconds after the onset (default 0.02,16)")
    ap.add_argument("--array", metavar="X,Z,GAIN,DELAY[;X,Z,GAIN,DELAY...]", type=array_members, action="append", default=[],
                    help="a source array, repeatable (one array per flag, at most %d of at most %d members): the combined response "
                         "at the listener of members at x, z with a gain (negative: polarity) and a delay in seconds, mixed on the "
                         "GPU; adds an \"arrays\" list with each array's onset and its records of --room-metrics, --decay-times, "
                         "--echo-criterion, --bands, --modulation and --spectrum; works with and without --sparse-emitters (there "
                         "the members' positions are added to the registered emitters)" % (api.ARRAYS_MAX, api.ARRAY_MEMBERS_MAX))
    ap.add_argument("--array-interp", choices=("nearest", "lagrange3"), default="lagrange3",
                    help="with --array: a member's delay rounded to a step, or a third-order Lagrange fractional delay (default)")
    ap.add_argument("--auralise", metavar="SIGNAL.npy|SIGNAL.wav",
                    help="render a dry mono signal at --aural-rate (a 1-D .npy, or a 16-bit PCM mono .wav of that rate) through the "
                         "recorded responses, resampled and convolved on the GPU: through every --array's response, else through the "
                         "response at every emitter's cell, mixed with gain 1; writes the mix to --aural-out and adds an "
                         "\"auralisation\" object; works with and without --sparse-emitters (at most %d receivers)"
                         % api.AURAL_MAX_RECEIVERS)
    ap.add_argument("--aural-rate", type=int, default=48000, help="with --auralise: the audio rate in samples per second (default 48000)")
    ap.add_argument("--aural-window", metavar="Z,BETA", type=echogram_window, default=(16, 9.0),
                    help="with --auralise: the resampler's zero crossings per side and Kaiser beta (default 16,9)")
    ap.add_argument("--aural-out", metavar="OUT.npy|OUT.wav", default="auralised.npy",
                    help="with --auralise: where the mix goes: float32 .npy, or a peak-normalised 16-bit PCM .wav (default auralised.npy)")
    ap.add_argument("--bands", metavar="HZ[,HZ...]", type=lambda v: [float(x) for x in v.split(",")],
                    help="add the band metrics (decay times and clarity of the band-filtered response) of each emitter's cell for "
                         "the bands centred at these frequencies")
    ap.add_argument("--band-fraction", type=int, default=1, choices=(1, 3), help="octave (1, default) or third-octave (3) bands")
    ap.add_argument("--modulation", action="store_true",
                    help="with --bands: add the modulation transfer function (m at the 14 IEC modulation frequencies) and the "
                         "modulation transfer index of each band at each emitter's cell")
    ap.add_argument("--in-run-records", action="store_true",
                    help="take the room metrics, decay times, lateral fraction, echogram, echo criterion and lobes -- and the band "
                         "metrics, modulation and spectrum of --bands, --modulation and --spectrum -- from records computed inside "
                         "the run for the emitters' cells (at most 64 emitters) instead of from whole-map passes after it; the "
                         "output is the same")
    ap.add_argument("--sparse-emitters", action="store_true",
                    help="run in sparse-emitter mode (streaming_analysis = 1: a ring of pressure planes instead of the history, the "
                         "mode of the large grids) with the emitters registered, and take the same records as --in-run-records "
                         "from the emitter records computed inside the run from per-emitter traces (at most 1024 emitters); the "
                         "output is the same")
    ap.add_argument("--emission-records", action="store_true",
                    help="add all six record kinds of each emitter as the LIVE module serves them by emission id "
                         "(PlaneverbSetEmissionRecords; --echogram and --lobes give their settings, default 0.005,16 and "
                         "0.01,0.08), under the key names of --in-run-records")
    ap.add_argument("--zone", metavar="XMIN,ZMIN,XMAX,ZMAX", type=rect4, action="append", default=[],
                    help="a receiver area in metres (repeatable, at most 64; a later one overwrites an earlier one where they "
                         "overlap): with any of the map options above, add a table per zone with n, mean, std, min and max of "
                         "every plane of those maps over the zone's cells, reduced on the GPU; with --zone-decay, the zone's "
                         "ensemble decay curve and its decay times; with --sparse-emitters only --zone-decay absolute, whose "
                         "curves are accumulated inside the run, and the tables of --room-metrics and --spectrum, whose records "
                         "of the zones' cells are too (no tables of the other maps: that mode keeps no history)")
    ap.add_argument("--zone-decay", choices=api.ZONE_DECAY_ALIGN_NAMES,
                    help="with --zone (it counts as one of the options --zone needs): add per zone the ensemble decay curve's table "
                         "-- the squared responses of the zone's reached cells summed on the GPU, by time since emission (absolute) "
                         "or since each cell's onset (onset) --: nCells, tFirst, tLast, EDT, T20, T30, depth and the point counts")
    ap.add_argument("--zone-decay-curves", action="store_true",
                    help="with --zone-decay: add the curves themselves, etc (energy per step) and edc (its backward sum)")
    ap.add_argument("--zone-band-decay", action="store_true",
                    help="with --zone-decay and --bands: add per zone a zoneBandDecay list, one entry per band -- the ensemble decay "
                         "curve of the band-filtered responses, reduced on the GPU in the alignment of --zone-decay: EDT, T20, T30, "
                         "depth, the point counts and the curve's C50, C80, D50 and Ts (with --zone-decay-curves: etc and edc too)")
    ap.add_argument("--mesh", metavar="FILE.npz[,ABSORPTION[,shell:R]]", type=mesh_setting, action="append", default=[],
                    help="a triangle mesh on top of the scene's boxes, repeatable: an .npz with `vertices` (nv x 3 world x, y, z; y is "
                         "the height) and `triangles` (nt x 3 indices), sliced at --slice-height and rasterised on the GPU; solid "
                         "(the section is filled, holes included; the mesh must be closed) unless shell:R is given (cells within "
                         "R metres of the section).  Absorption as in a .pv box, default 0.5")
    ap.add_argument("--slice-height", type=float, default=0.0, help="world height at which the meshes are sliced, default 0")
    ap.add_argument("--save", help="write the loaded boxes back as a .pv file and exit (no GPU needed)")
    a = ap.parse_args(argv)

    if a.modulation and not a.bands:
        ap.error("--modulation: needs --bands")
    if a.zone and a.in_run_records:
        ap.error("--zone: reduces the whole-map passes (not with --in-run-records)")
    if a.zone and a.sparse_emitters and (a.zone_band_decay or a.zone_decay == "onset" or
                                         not (a.zone_decay or a.room_metrics or a.spectrum)):
        ap.error("--zone: with --sparse-emitters only --zone-decay absolute, --room-metrics and --spectrum (the curves and those two "
                 "maps are accumulated inside the run; the onset-synchronised and the band curves and the other maps need the history)")
    if a.in_run_records and a.sparse_emitters:
        ap.error("--sparse-emitters: not with --in-run-records (the output queries' records need the history)")
    if a.zone_decay and not a.zone:
        ap.error("--zone-decay: needs --zone")
    if a.zone_decay_curves and not a.zone_decay:
        ap.error("--zone-decay-curves: needs --zone-decay")
    if a.zone_band_decay and not (a.zone_decay and a.bands):
        ap.error("--zone-band-decay: needs --zone-decay and --bands")
    if len(a.zone) > api.ZONES_MAX:
        ap.error("--zone: at most %d zones" % api.ZONES_MAX)
    boxes = api.load_pv(a.scene)
    if a.save:
        api.save_pv(a.save, boxes)
        print(json.dumps({"saved": a.save, "boxes": len(boxes)}))
        return 0
    size = a.size
    if a.cells:
        dx = np.float32(343.21) / np.float32(a.res) / np.float32(3.5)
        size = float((a.cells + 0.5) * dx)
    emitters = a.emitter or [(5.0, 0.0, 6.0)]
    if a.in_run_records and len(emitters) > 64:
        ap.error("--in-run-records: at most 64 emitters (a run's output queries)")
    if a.sparse_emitters and len(emitters) > api.RECORD_QUERIES_MAX:
        ap.error("--sparse-emitters: at most %d emitters" % api.RECORD_QUERIES_MAX)
    if a.waterfall is not None and len(emitters) > api.WATERFALL_MAX_RECEIVERS:
        ap.error("--waterfall: at most %d emitters" % api.WATERFALL_MAX_RECEIVERS)
    if a.auralise:
        if not a.array and len(emitters) > api.AURAL_MAX_RECEIVERS:
            ap.error("--auralise: at most %d emitters" % api.AURAL_MAX_RECEIVERS)
        try:
            signal = read_signal(a.auralise, a.aural_rate)
        except Exception as e:  # (an unreadable file, wave.Error, a shape or a rate that does not fit)
            ap.error("--auralise: %s" % e)
    with api.Solver(size, size, a.res, device=a.device, **(dict(streaming_analysis=1) if a.sparse_emitters else {})) as s:
        for b in boxes:
            s.add_geometry(b)
        s.set_slice_height(a.slice_height)
        for path, absorption, mode, radius in a.mesh:
            with np.load(path) as f:
                s.add_mesh(f["vertices"], f["triangles"], absorption, mode, radius)
        # the record kinds from whole-map passes after the run, or from inside the run
        whole = not (a.in_run_records or a.sparse_emitters)
        if not whole:
            kinds = ((api.QREC_ROOM_METRICS if a.room_metrics else 0) | (api.QREC_DECAY_TIMES if a.decay_times else 0) |
                     (api.QREC_LATERAL if a.lateral_fraction else 0) | (api.QREC_ECHOGRAM if a.echogram else 0) |
                     (api.QREC_ECHO_CRITERION if a.echo_criterion else 0) | (api.QREC_LOBES if a.lobes is not None else 0))
            if a.echogram:
                s.set_echogram(*a.echogram)
            if a.lobes is not None:
                s.set_lobe_windows(a.lobes)
            spectral = ((api.QSPEC_BAND_METRICS if a.bands else 0) | (api.QSPEC_MODULATION if a.modulation else 0) |
                        (api.QSPEC_SPECTRUM if a.spectrum else 0))
            if a.bands:
                s.set_bands(a.bands, a.band_fraction)
            if a.spectrum:
                s.set_spectrum_bins(a.spectrum)
            if a.sparse_emitters:
                # (the members of --array read the traces of registered emitters: theirs follow the emitters asked for)
                s.set_emitters(list(emitters) + [m[0] for arr in a.array for m in arr])
                s.set_emitter_records(kinds, spectral)
                if a.zone:  # (the curves of --zone-decay absolute are accumulated inside the run)
                    s.set_zones(api.zone_labels_from_rects(s.dx, s.gx, s.gy, a.zone), len(a.zone))
                    if a.zone_decay:
                        s.set_zone_curves(True)
                    # (... and so are the room-metrics and spectrum records of the zones' cells)
                    s.set_zone_maps((api.ZMAP_ROOM_METRICS if a.room_metrics else 0) | (api.ZMAP_SPECTRUM if a.spectrum else 0))
            else:
                s.set_output_queries(emitters)
                s.set_query_records(kinds)
                s.set_query_spectral_records(spectral)
        s.run(a.listener)
        spec_per = {api.QSPEC_BAND_METRICS: 12, api.QSPEC_MODULATION: 15, api.QSPEC_SPECTRUM: 3}
        if a.sparse_emitters:
            # set_emitters keeps the positions on the map, in order: row i of the output is the kept emitter's record, or NaNs
            on_map = [api.host_cells(size, size, a.res, e[0], e[2])[1] is not None for e in emitters]
            row = np.cumsum(on_map) - 1

            def per_position(r):
                full = np.full((len(emitters),) + r.shape[1:], np.nan, np.float32)
                full[np.flatnonzero(on_map)] = r[row[np.flatnonzero(on_map)]]
                return full

            qrec = dict((k, per_position(s.emitter_records(k))) for k in RECORD_KEYS if kinds & k)
            qspec = dict((k, per_position(s.emitter_records(k, spectral=True).reshape(s.emitter_cells().shape[0], -1, spec_per[k])))
                         for k in spec_per if spectral & k)
        else:
            qrec = {} if whole else dict((k, s.queried_records(k)) for k in RECORD_KEYS if kinds & k)
            qspec = {} if whole else dict((k, s.queried_spectral_records(k)) for k in spec_per if spectral & k)
        t = s.timings()
        out = {"scene": a.scene, "grid": [s.gx, s.gy], "T": s.T, "res": a.res, "dx": s.dx, "efree": s.efree,
               "listener": a.listener, "fdtd_ms": t.fdtdMs, "analysis_ms": t.analysisMs, "emitters": []}
        if whole and a.room_metrics:
            s.compute_room_metrics()
        if whole and a.decay_times:
            s.compute_decay_times()
        if whole and a.echo_criterion:
            s.compute_echo_criterion()
        if whole and a.lateral_fraction:
            s.compute_lateral_fraction()
        if whole and a.echogram:
            s.set_echogram(*a.echogram)
            s.compute_echogram()
        if whole and a.lobes is not None:
            s.set_lobe_windows(a.lobes)
            s.compute_lobes()
        if whole and a.bands:
            s.set_bands(a.bands, a.band_fraction)
            s.compute_band_metrics()
        if whole and a.modulation:
            s.compute_modulation()
        if whole and a.spectrum:
            s.set_spectrum_bins(a.spectrum)
            s.compute_spectrum()
        if a.waterfall is not None:  # (one pass over the emitters' cells: the history, or in sparse-emitter mode the traces)
            s.set_waterfall(a.waterfall, *a.waterfall_slices)
            s.compute_waterfall(None if a.sparse_emitters else emitters)
            wf = s.waterfall()
            if a.sparse_emitters:
                wf = dict((k, per_position(v)) for k, v in wf.items())
            wf_hz, wf_seconds, wf_steps, _ = s.waterfall_setting()
        if a.array:  # (one mix of the members' responses per array: off the history, or in sparse-emitter mode off the traces)
            # (the bands and the bins are set by now: in front of the run, or with the whole-map passes above)
            s.set_arrays(a.array, api.ARRAY_NEAREST if a.array_interp == "nearest" else api.ARRAY_LAGRANGE3)
            s.set_array_records((api.QREC_ROOM_METRICS if a.room_metrics else 0) | (api.QREC_DECAY_TIMES if a.decay_times else 0) |
                                (api.QREC_ECHO_CRITERION if a.echo_criterion else 0),
                                (api.QSPEC_BAND_METRICS if a.bands else 0) | (api.QSPEC_MODULATION if a.modulation else 0) |
                                (api.QSPEC_SPECTRUM if a.spectrum else 0))
            s.compute_arrays()
            onsets = s.array_onsets()
            out["arrays"] = []
            for i, arr in enumerate(a.array):
                tm, td, tw = s.array_taps(i)
                rec = {"members": [{"position": list(m[0]), "gain": m[1], "delaySeconds": m[2]} for m in arr], "interp": a.array_interp,
                       "taps": {"member": [int(v) for v in tm], "delaySteps": [int(v) for v in td], "weight": [float(v) for v in tw]},
                       "onset": float(onsets[i]) if onsets[i] < 1e30 else None}
                out["arrays"].append(rec)
            if a.room_metrics:
                for rec, m in zip(out["arrays"], s.array_records(api.QREC_ROOM_METRICS)):
                    rec["roomMetrics"] = dict((n, float(v)) for n, v in zip(api.ROOM_METRIC_NAMES, m))
            if a.decay_times:
                for rec, m in zip(out["arrays"], s.array_records(api.QREC_DECAY_TIMES)):
                    rec["decayTimes"] = dict((n, float(v)) for n, v in zip(api.DECAY_TIME_NAMES, m))
            if a.echo_criterion:
                for rec, m in zip(out["arrays"], s.array_records(api.QREC_ECHO_CRITERION)):
                    rec["echoCriterion"] = dict((n, float(v)) for n, v in zip(api.ECHO_CRITERION_NAMES, m))
            if a.bands:
                for rec, m in zip(out["arrays"], s.array_records(api.QSPEC_BAND_METRICS, spectral=True).reshape(len(a.array), -1, 12)):
                    rec["bandMetrics"] = [
                        dict([("hz", float(hz)), ("fraction", a.band_fraction)] + [(n, float(v)) for n, v in zip(api.BAND_METRIC_NAMES, r)])
                        for hz, r in zip(a.bands, m)]
            if a.modulation:
                for rec, m in zip(out["arrays"], s.array_records(api.QSPEC_MODULATION, spectral=True).reshape(len(a.array), -1, 15)):
                    rec["modulation"] = {
                        "hz": [float(v) for v in s.modulation_frequencies()],
                        "bands": [{"hz": float(hz), "fraction": a.band_fraction, "m": [float(v) for v in r[:-1]], "mti": float(r[-1])}
                                  for hz, r in zip(a.bands, m)]}
            if a.spectrum:
                for rec, m in zip(out["arrays"], s.array_records(api.QSPEC_SPECTRUM, spectral=True).reshape(len(a.array), -1, 3)):
                    rec["spectrum"] = {"hz": [float(v) for v in s.spectrum_bins()], "re": [float(v) for v in m[:, 0]],
                                       "im": [float(v) for v in m[:, 1]], "levelDb": [float(v) for v in m[:, 2]]}
        if a.auralise:  # (the signal through every array's response, else through the response at every emitter's cell; then the mix)
            s.set_auralisation(a.aural_rate, *a.aural_window)
            if a.array:
                s.compute_aural_responses(source=api.AURAL_ARRAYS)
                count = len(a.array)
            elif a.sparse_emitters:
                s.compute_aural_responses()
                count = len(s.emitter_cells())
            else:
                kept = [e for e in emitters if api.host_cells(size, size, a.res, e[0], e[2])[1] is not None]
                if not kept:
                    ap.error("--auralise: no emitter on the map")
                s.compute_aural_responses(kept)
                count = len(kept)
            ms = s.auralise(signal, [0] * count)
            mix = s.aural_mix()
            write_signal(a.aural_out, mix, a.aural_rate)
            _, _, _, aural_l, aural_k = s.auralisation_setting()
            out["auralisation"] = {"rate": a.aural_rate, "zeroCrossings": a.aural_window[0], "beta": a.aural_window[1],
                                   "source": "arrays" if a.array else "emitters", "receivers": count, "signalSamples": int(signal.size),
                                   "responseSamples": aural_l, "tapsPerSample": aural_k, "samples": int(mix.size),
                                   "peak": float(np.abs(mix).max()), "convolve_ms": ms, "out": a.aural_out}
        for i, e in enumerate(emitters):
            o = s.get_output(e)
            ga, gb, gc = api.reverb_bus_gains(o.rt60, o.wetGain)
            out["emitters"].append({
                "position": e, "occlusion": o.occlusion, "wetGain": o.wetGain, "rt60": o.rt60, "lowpass": o.lowpass,
                "direction": [o.directionX, o.directionY], "sourceDirectivity": [o.sourceDirectionX, o.sourceDirectionY],
                "reverbBusGains": [ga, gb, gc]})
            if a.room_metrics:
                m = s.room_metrics_at(e) if whole else qrec[api.QREC_ROOM_METRICS][i]
                out["emitters"][-1]["roomMetrics"] = dict((n, float(v)) for n, v in zip(api.ROOM_METRIC_NAMES, m))
            if a.decay_times:
                m = s.decay_times_at(e) if whole else qrec[api.QREC_DECAY_TIMES][i]
                out["emitters"][-1]["decayTimes"] = dict((n, float(v)) for n, v in zip(api.DECAY_TIME_NAMES, m))
            if a.echo_criterion:
                m = s.echo_criterion_at(e) if whole else qrec[api.QREC_ECHO_CRITERION][i]
                out["emitters"][-1]["echoCriterion"] = dict((n, float(v)) for n, v in zip(api.ECHO_CRITERION_NAMES, m))
            if a.lateral_fraction:
                m = s.lateral_fraction_at(e) if whole else qrec[api.QREC_LATERAL][i]
                out["emitters"][-1]["lateralFraction"] = dict((n, float(v)) for n, v in zip(api.LATERAL_FRACTION_NAMES, m))
            if a.echogram:
                m = s.echogram_at(e) if whole else qrec[api.QREC_ECHOGRAM][i]
                out["emitters"][-1]["echogram"] = {"slotSteps": s.echogram_slots()[2], "n": float(m[0]),
                                                   "e": [float(v) for v in m[1::3]], "ix": [float(v) for v in m[2::3]],
                                                   "iy": [float(v) for v in m[3::3]]}
            if a.lobes is not None:
                m = s.lobes_at(e) if whole else qrec[api.QREC_LOBES][i]
                out["emitters"][-1]["lobes"] = {"n": float(m[0]), "windows": [
                    dict((n, float(v)) for n, v in zip(api.LOBE_NAMES, m[1 + 5 * w:6 + 5 * w])) for w in range((len(m) - 1) // 5)]}
            if a.bands:
                m = s.band_metrics_at(e) if whole else qspec[api.QSPEC_BAND_METRICS][i]
                out["emitters"][-1]["bandMetrics"] = [
                    dict([("hz", float(hz)), ("fraction", a.band_fraction)] + [(n, float(v)) for n, v in zip(api.BAND_METRIC_NAMES, r)])
                    for hz, r in zip(a.bands, m)]
            if a.modulation:
                m = s.modulation_at(e) if whole else qspec[api.QSPEC_MODULATION][i]
                out["emitters"][-1]["modulation"] = {
                    "hz": [float(v) for v in s.modulation_frequencies()],
                    "bands": [{"hz": float(hz), "fraction": a.band_fraction, "m": [float(v) for v in r[:-1]], "mti": float(r[-1])}
                              for hz, r in zip(a.bands, m)]}
            if a.spectrum:
                m = s.spectrum_at(e) if whole else qspec[api.QSPEC_SPECTRUM][i]
                out["emitters"][-1]["spectrum"] = {"hz": [float(v) for v in s.spectrum_bins()], "re": [float(v) for v in m[:, 0]],
                                                   "im": [float(v) for v in m[:, 1]], "levelDb": [float(v) for v in m[:, 2]]}
            if a.waterfall is not None:
                out["emitters"][-1]["waterfall"] = {
                    "hz": [float(v) for v in wf_hz], "sliceSeconds": wf_seconds, "sliceSteps": wf_steps, "onset": float(wf["onset"][i]),
                    "re": [float(v) for v in wf["response"][i, :, 0]], "im": [float(v) for v in wf["response"][i, :, 1]],
                    "levelDb": [[float(v) for v in row] for row in wf["level"][i]]}
        if a.zone:
            out["zones"] = zone_tables(s, a)
        if a.emission_records:
            echogram = a.echogram or (0.005, 16)
            s.set_echogram(*echogram)  # (for the slot length in steps)
            slot_steps = s.echogram_slots()[2]
    if a.emission_records:
        live = live_emission_records(size, a.res, boxes, a.listener, emitters, echogram, a.lobes or None, slot_steps)
        for e, r in zip(out["emitters"], live):
            e.update(r)
    print(json.dumps(out, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
