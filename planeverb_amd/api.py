"""ctypes binding of libplaneverb_amd.so -- the host-side mirror of Planeverb's interface for the FDTD path.

Two layers, both thin:

* module-level functions `Init / Exit / Emit / UpdateEmission / EndEmission / GetOutput / AddGeometry /
  UpdateGeometry / RemoveGeometry / SetListenerPosition` with the names, argument meaning and sentinel behaviour of
  the reference's C++ API (ProjectPlaneverb/include/Planeverb.h:12-47) on top of the flat C-ABI
  (PlaneverbUnityPluginAPI/PlaneverbUnity.cpp:25-135);
* `Solver`, the synchronous batch handle (PvAmd* extension) used by the benchmarks, the parity tests and the
  multi-GPU sharding layer.

There is no CPU implementation behind this module: if the shared library is missing it raises, and if no HIP device
is visible every call that needs one fails loudly.
"""
import ctypes as C
import os
from collections import namedtuple

import numpy as np

from .build import LIB_PATH

PV_INVALID_DRY_GAIN = -1.0
PV_INVALID_ID = -1

PVA_OPT_DENSE_HISTORY = 1
PVA_OPT_NUM_STEPS = 2
PVA_OPT_SKIP_ANALYSIS = 3
PVA_OPT_USE_GRAPH = 4
PVA_OPT_STEPS_PER_LAUNCH = 5
PVA_OPT_TILE_ROWS = 6
PVA_OPT_NO_FREE_GRID = 7
PVA_OPT_TIME_KERNELS = 8
PVA_OPT_TILE_ORDER = 9
PVA_OPT_SMALL_GRID_KERNEL = 10
PVA_OPT_PACKED_MATH = 11
PVA_OPT_STREAMING_ANALYSIS = 12
PVA_OPT_STREAM_ROWS = 13
PVA_OPT_MERGED_LAUNCH = 14
PVA_OPT_EDGE_TILES = 15
PVA_OPT_ROW_BANDS = 16
PVA_OPT_PATCH_KERNEL = 17
PVA_OPT_PATCH_STRIP = 18
PVA_OPT_LAZY_FAR_CELLS = 19
PVA_OPT_STREAM_FUSE = 20
PVA_OPT_AUX_STREAMS = 21
PVA_OPT_RESIDENT_KERNEL = 22
PVA_OPT_RT60_LANES = 23
PVA_OPT_DEBUG_LOSE_FIRST_CAPTURE = 24
PVA_OPT_STREAM_PRIORITY = 25
PVA_OPT_ALTERNATE_SWEEPS = 26
PVA_OPT_XCD_REGIONS = 27
PVA_OPT_ANALYSIS_FORK = 28
PVA_OPT_FUSED_ANALYSIS = 29
PVA_OPT_REACH_BOUND = 30
PVA_OPT_RESIDENT_WINDOW = 31


class PlaneverbOutput(C.Structure):
    """PlaneverbUnity.cpp:66-76"""
    _fields_ = [("occlusion", C.c_float), ("wetGain", C.c_float), ("rt60", C.c_float), ("lowpass", C.c_float),
                ("directionX", C.c_float), ("directionY", C.c_float), ("sourceDirectionX", C.c_float),
                ("sourceDirectionY", C.c_float)]

    def as_array(self):
        return np.array([self.occlusion, self.wetGain, self.rt60, self.lowpass, self.directionX, self.directionY,
                         self.sourceDirectionX, self.sourceDirectionY], np.float32)


class PlaneverbCell(C.Structure):
    """PvTypes.h:106-121"""
    _fields_ = [("pr", C.c_float), ("vx", C.c_float), ("vy", C.c_float), ("b", C.c_short), ("by", C.c_short)]


CELL_DTYPE = np.dtype([("pr", np.float32), ("vx", np.float32), ("vy", np.float32), ("b", np.int16), ("by", np.int16)])


class PvAmdInfo(C.Structure):
    _fields_ = [("gx", C.c_int), ("gy", C.c_int), ("T", C.c_int), ("fs", C.c_int), ("res", C.c_int),
                ("dx", C.c_float), ("dt", C.c_float), ("efree", C.c_float), ("device", C.c_int),
                ("stepsPerLaunch", C.c_int), ("tileRows", C.c_int), ("tileCols", C.c_int), ("pitch", C.c_int),
                ("rows", C.c_int), ("histRows", C.c_int), ("histPitch", C.c_int), ("numGeometry", C.c_int),
                ("deviceBytes", C.c_longlong), ("streamFuse", C.c_int), ("residentKernel", C.c_int)]


class PvAmdBakeInfo(C.Structure):
    _fields_ = [("gx", C.c_int), ("gy", C.c_int), ("T", C.c_int), ("fs", C.c_int), ("res", C.c_int), ("dx", C.c_float),
                ("stride", C.c_int), ("x0", C.c_float), ("z0", C.c_float), ("sx", C.c_float), ("sz", C.c_float),
                ("nx", C.c_int), ("nz", C.c_int), ("probesBaked", C.c_int), ("probesInvalid", C.c_int),
                ("records", C.c_longlong), ("materialHash", C.c_ulonglong)]


class PvAmdSlabInfo(C.Structure):
    _fields_ = [("nslabs", C.c_int), ("row0", C.c_int * 16), ("rows", C.c_int * 16), ("device", C.c_int * 16),
                ("haloBytesPerLaunch", C.c_longlong), ("exchangeBytesPerRun", C.c_longlong),
                ("deviceBytes", C.c_longlong * 16), ("handoffWords", C.c_int), ("streamRedeals", C.c_int),
                ("dryRunUsPerSweep", C.c_float)]


class PvAmdTimings(C.Structure):
    _fields_ = [("fdtdMs", C.c_float), ("analysisMs", C.c_float), ("geometryMs", C.c_float),
                ("stepKernelMs", C.c_float), ("stepLaunches", C.c_int), ("airKernelMs", C.c_float), ("generalKernelMs", C.c_float), ("airLaunches", C.c_int),
                ("generalLaunches", C.c_int), ("stepLoopMs", C.c_float), ("reachedCells", C.c_int), ("activeCells", C.c_int), ("silentCells", C.c_int)]


ROOM_METRIC_NAMES = ("c50", "c80", "d50", "ts", "e50", "l50", "e80", "l80", "total", "moment")


class PvAmdRoomMetrics(C.Structure):
    _fields_ = [(n, C.c_float) for n in ROOM_METRIC_NAMES]

    def as_array(self):
        return np.frombuffer(self, np.float32).copy()


DECAY_TIME_NAMES = ("edt", "t20", "t30", "n_edt", "n_t20", "n_t30", "e0", "depth")


class PvAmdDecayTimes(C.Structure):
    _fields_ = [(n, C.c_float) for n in DECAY_TIME_NAMES]

    def as_array(self):
        return np.frombuffer(self, np.float32).copy()


LATERAL_FRACTION_NAMES = ("lf", "dir_x", "dir_y", "n", "e80", "lateral", "fx", "fy", "sxx", "sxy", "syy")


class PvAmdLateralFraction(C.Structure):
    _fields_ = [(n, C.c_float) for n in LATERAL_FRACTION_NAMES]

    def as_array(self):
        return np.frombuffer(self, np.float32).copy()


ECHO_CRITERION_NAMES = ("s_ek", "s_tk", "s_ek_late", "s_tk_late", "s_ts", "m_ek", "m_tk", "m_ek_late", "m_tk_late", "m_ts")
ECHO_SPEECH_CRIT = 1.0  # PVA_ECHO_SPEECH_CRIT
ECHO_MUSIC_CRIT = 1.8   # PVA_ECHO_MUSIC_CRIT


class PvAmdEchoCriterion(C.Structure):
    _fields_ = [(n, C.c_float) for n in ("sEk", "sTk", "sEkLate", "sTkLate", "sTs", "mEk", "mTk", "mEkLate", "mTkLate", "mTs")]

    def as_array(self):
        return np.frombuffer(self, np.float32).copy()


# every symbol include/planeverb_amd.h declares: name -> (restype, argtypes)
_fp = C.POINTER(C.c_float)
_vp = C.c_void_p
SYMBOLS = {
    "UnityPluginLoad": (None, [_vp]),
    "UnityPluginUnload": (None, []),
    "PlaneverbInit": (None, [C.c_float, C.c_float, C.c_int, C.c_int, C.c_char_p, C.c_int, C.c_int]),
    "PlaneverbExit": (None, []),
    "PlaneverbEmit": (C.c_int, [C.c_float] * 3),
    "PlaneverbUpdateEmission": (None, [C.c_int] + [C.c_float] * 3),
    "PlaneverbEndEmission": (None, [C.c_int]),
    "PlaneverbGetOutput": (PlaneverbOutput, [C.c_int]),
    "PlaneverbAddGeometry": (C.c_int, [C.c_float] * 5),
    "PlaneverbUpdateGeometry": (None, [C.c_int] + [C.c_float] * 5),
    "PlaneverbRemoveGeometry": (None, [C.c_int]),
    "PlaneverbSetListenerPosition": (None, [C.c_float] * 3),
    "PlaneverbAddOrientedGeometry": (C.c_int, [C.c_float] * 7),
    "PlaneverbUpdateOrientedGeometry": (None, [C.c_int] + [C.c_float] * 7),
    "PlaneverbRemoveOrientedGeometry": (None, [C.c_int]),
    "PlaneverbAddPolygonGeometry": (C.c_int, [_fp, C.c_int, C.c_float]),
    "PlaneverbUpdatePolygonGeometry": (None, [C.c_int, _fp, C.c_int, C.c_float]),
    "PlaneverbRemovePolygonGeometry": (None, [C.c_int]),
    "PlaneverbAddDiscGeometry": (C.c_int, [C.c_float] * 4),
    "PlaneverbUpdateDiscGeometry": (None, [C.c_int] + [C.c_float] * 4),
    "PlaneverbRemoveDiscGeometry": (None, [C.c_int]),
    "PlaneverbAddWallPathGeometry": (C.c_int, [_fp, C.c_int, C.c_float, C.c_float]),
    "PlaneverbUpdateWallPathGeometry": (None, [C.c_int, _fp, C.c_int, C.c_float, C.c_float]),
    "PlaneverbRemoveWallPathGeometry": (None, [C.c_int]),
    "PlaneverbAddConcavePolygonGeometry": (C.c_int, [_fp, C.c_int, C.c_float]),
    "PlaneverbUpdateConcavePolygonGeometry": (None, [C.c_int, _fp, C.c_int, C.c_float]),
    "PlaneverbRemoveConcavePolygonGeometry": (None, [C.c_int]),
    "PlaneverbAddMeshGeometry": (C.c_int, [_fp, C.c_int, C.POINTER(C.c_int), C.c_int, C.c_float, C.c_int, C.c_float]),
    "PlaneverbSetMeshGeometryTransform": (None, [C.c_int, _fp]),
    "PlaneverbRemoveMeshGeometry": (None, [C.c_int]),
    "PlaneverbSetSliceHeight": (None, [C.c_float]),
    "PlaneverbLoadScene": (C.c_int, [C.c_char_p]),
    "PlaneverbIterationCount": (C.c_longlong, []),
    "PlaneverbWaitIterations": (C.c_longlong, [C.c_longlong, C.c_int]),
    "PlaneverbIsRunning": (C.c_int, []),
    "PlaneverbWorkerError": (C.c_char_p, []),
    "PlaneverbIsStreaming": (C.c_int, []),
    "PlaneverbGetImpulseResponse": (C.c_int, [C.c_float] * 3 + [C.POINTER(PlaneverbCell), C.c_int]),
    "PlaneverbSetEmissionRecords": (C.c_int, [C.c_uint]),
    "PlaneverbSetEmissionEchogram": (C.c_int, [C.c_float, C.c_int]),
    "PlaneverbSetEmissionLobeWindows": (C.c_int, [_fp, C.c_int]),
    "PlaneverbEmissionRecordKinds": (C.c_uint, []),
    "PlaneverbEmissionRecordFloats": (C.c_int, [C.c_uint]),
    "PlaneverbEmissionRecordCells": (C.c_int, []),
    "PlaneverbGetEmissionRecord": (C.c_int, [C.c_int, C.c_uint, _fp, C.c_int]),
    "PvAmdDeviceCount": (C.c_int, []),
    "PvAmdLastError": (C.c_char_p, []),
    "PvAmdVersion": (C.c_char_p, []),
    "PvAmdCreate": (_vp, [C.c_float, C.c_float, C.c_int, C.c_int]),
    "PlaneverbCreateGrid": (_vp, [C.c_float, C.c_float, C.c_int, C.c_int]),
    "PvAmdCreateSlabs": (_vp, [C.c_float, C.c_float, C.c_int, C.POINTER(C.c_int), C.c_int]),
    "PvAmdGetSlabInfo": (C.c_int, [_vp, C.POINTER(PvAmdSlabInfo)]),
    "PvAmdCreateSlabRank": (_vp, [C.c_float, C.c_float, C.c_int, C.c_int, C.c_int, C.c_int]),
    "PvAmdComputeEfree": (C.c_int, [C.c_float, C.c_float, C.c_int, C.c_int, _fp]),
    "PvAmdSlabSetEfree": (C.c_int, [_vp, C.c_float]),
    "PvAmdSlabBegin": (C.c_int, [_vp] + [C.c_float] * 3),
    "PvAmdSlabNumLaunches": (C.c_int, [_vp]),
    "PvAmdSlabLaunch": (C.c_int, [_vp, C.c_int]),
    "PvAmdSlabHaloFloats": (C.c_int, [_vp]),
    "PvAmdSlabExportHalo": (C.c_int, [_vp, C.c_int, _fp]),
    "PvAmdSlabImportHalo": (C.c_int, [_vp, C.c_int, _fp]),
    "PvAmdSlabHistoryFloats": (C.c_int, [_vp]),
    "PvAmdSlabExportEdgeHistory": (C.c_int, [_vp, _fp]),
    "PvAmdSlabImportAboveHistory": (C.c_int, [_vp, _fp]),
    "PvAmdSlabAnalyze": (C.c_int, [_vp]),
    "PvAmdSlabWindowBlock": (C.c_longlong, [_vp, C.POINTER(C.c_int), _fp, C.c_longlong]),
    "PvAmdSlabRootCreate": (_vp, [_vp, C.c_int]),
    "PvAmdSlabRootDestroy": (None, [_vp]),
    "PvAmdSlabRootBegin": (C.c_int, [_vp] + [C.c_float] * 3),
    "PvAmdSlabRootImportBlock": (C.c_int, [_vp, C.POINTER(C.c_int), _fp]),
    "PvAmdSlabRootFinish": (C.c_int, [_vp]),
    "PvAmdSlabRootGetOutput": (C.c_int, [_vp] + [C.c_float] * 3 + [C.POINTER(PlaneverbOutput)]),
    "PvAmdSlabRootCopyResults": (C.c_int, [_vp, _fp, _fp]),
    "PvAmdDestroy": (None, [_vp]),
    "PvAmdSetOption": (C.c_int, [_vp, C.c_int, C.c_longlong]),
    "PvAmdGetInfo": (C.c_int, [_vp, C.POINTER(PvAmdInfo)]),
    "PvAmdAddGeometry": (C.c_int, [_vp] + [C.c_float] * 5),
    "PvAmdUpdateGeometry": (C.c_int, [_vp, C.c_int] + [C.c_float] * 5),
    "PvAmdRemoveGeometry": (C.c_int, [_vp, C.c_int]),
    "PvAmdLoadScene": (C.c_int, [_vp, C.c_char_p]),
    "PvAmdSaveScene": (C.c_int, [_vp, C.c_char_p]),
    "PvAmdAddShape": (C.c_int, [_vp, _fp, C.c_int, C.c_float]),
    "PvAmdUpdateShape": (C.c_int, [_vp, C.c_int, _fp, C.c_int, C.c_float]),
    "PvAmdRemoveShape": (C.c_int, [_vp, C.c_int]),
    "PvAmdAddOrientedBox": (C.c_int, [_vp] + [C.c_float] * 7),
    "PvAmdUpdateOrientedBox": (C.c_int, [_vp, C.c_int] + [C.c_float] * 7),
    "PvAmdAddDisc": (C.c_int, [_vp] + [C.c_float] * 4),
    "PvAmdUpdateDisc": (C.c_int, [_vp, C.c_int] + [C.c_float] * 4),
    "PvAmdAddCapsule": (C.c_int, [_vp] + [C.c_float] * 6),
    "PvAmdUpdateCapsule": (C.c_int, [_vp, C.c_int] + [C.c_float] * 6),
    "PvAmdAddWallPath": (C.c_int, [_vp, _fp, C.c_int, C.c_float, C.c_float]),
    "PvAmdUpdateWallPath": (C.c_int, [_vp, C.c_int, _fp, C.c_int, C.c_float, C.c_float]),
    "PvAmdAddPolygon": (C.c_int, [_vp, _fp, C.c_int, C.c_float]),
    "PvAmdUpdatePolygon": (C.c_int, [_vp, C.c_int, _fp, C.c_int, C.c_float]),
    "PvAmdAddMesh": (C.c_int, [_vp, _fp, C.c_int, C.POINTER(C.c_int), C.c_int, C.c_float, C.c_int, C.c_float]),
    "PvAmdUpdateMesh": (C.c_int, [_vp, C.c_int, _fp, C.c_int, C.POINTER(C.c_int), C.c_int, C.c_float, C.c_int, C.c_float]),
    "PvAmdSetMeshTransform": (C.c_int, [_vp, C.c_int, _fp]),
    "PvAmdRemoveMesh": (C.c_int, [_vp, C.c_int]),
    "PvAmdSetSliceHeight": (C.c_int, [_vp, C.c_float]),
    "PvAmdGetSliceHeight": (C.c_float, [_vp]),
    "PvAmdMeshTriangles": (C.c_int, [_vp, C.c_int]),
    "PvAmdCopyMeshSection": (C.c_int, [_vp, C.c_int, _fp, C.POINTER(C.c_ubyte)]),
    "PvAmdHostMeshSection": (C.c_int, [_fp, C.c_int, C.POINTER(C.c_int), C.c_int, _fp, C.c_float, _fp, C.POINTER(C.c_ubyte)]),
    "PvAmdHostMeshCoverage": (C.c_int, [C.c_float, C.c_float, C.c_int, _fp, C.c_int, C.POINTER(C.c_int), C.c_int, _fp, C.c_float,
                                        C.c_int, C.c_float, C.POINTER(C.c_ubyte)]),
    "PvAmdSetGridBoundary": (C.c_int, [_vp, _fp]),
    "PvAmdGetGridBoundary": (C.c_int, [_vp, _fp]),
    "PlaneverbSetGridBoundary": (None, [C.c_float] * 4),
    "PvAmdSetEdgeLayer": (C.c_int, [_vp, C.POINTER(C.c_int)]),
    "PvAmdGetEdgeLayer": (C.c_int, [_vp, C.POINTER(C.c_int)]),
    "PlaneverbSetEdgeLayer": (None, [C.c_int] * 4),
    "PvAmdSetEdgeLayerSplit": (C.c_int, [_vp, C.POINTER(C.c_int), C.c_double]),
    "PvAmdGetEdgeLayerModel": (C.c_int, [_vp, C.POINTER(C.c_int), C.POINTER(C.c_double)]),
    "PlaneverbSetEdgeLayerSplit": (None, [C.c_int] * 4),
    "PvAmdHostEdgeLayerTablesR0": (C.c_int, [C.c_float, C.c_float, C.c_int, C.POINTER(C.c_int), C.c_double, _fp]),
    "PvAmdHostEdgeLayerTables": (C.c_int, [C.c_float, C.c_float, C.c_int, C.POINTER(C.c_int), _fp]),
    "PvAmdHostEnclosure": (C.c_int, [C.POINTER(C.c_ubyte)] + [C.c_int] * 7 + [C.POINTER(C.c_int)]),
    "PvAmdHostOrientedBoxVertices": (C.c_int, [C.c_float] * 6 + [_fp]),
    "PvAmdHostShape": (C.c_int, [_fp, C.c_int, C.c_float, _fp]),
    "PvAmdHostShapeCoverage": (C.c_int, [C.c_float, C.c_float, C.c_int, _fp, C.c_int, C.POINTER(C.c_ubyte)]),
    "PvAmdHostRoundShapeCoverage": (C.c_int, [C.c_float, C.c_float, C.c_int, C.c_int, _fp, C.c_int, C.c_float,
                                              C.POINTER(C.c_ubyte)]),
    "PvAmdRun": (C.c_int, [_vp] + [C.c_float] * 3),
    "PvAmdRunAsync": (C.c_int, [_vp] + [C.c_float] * 3),
    "PvAmdRunAsyncAfter": (C.c_int, [_vp, _vp] + [C.c_float] * 3),
    "PvAmdSync": (C.c_int, [_vp]),
    "PvAmdRunBatch": (C.c_int, [C.POINTER(_vp), C.c_int, _fp, C.c_int]),
    "PvAmdGetTimings": (C.c_int, [_vp, C.POINTER(PvAmdTimings)]),
    "PvAmdLastRunResidentWindow": (C.c_int, [_vp]),
    "PvAmdLastRunOneXcd": (C.c_int, [_vp]),
    "PvAmdHostWindowClear": (C.c_int, [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int]),
    "PvAmdClockProbe": (C.c_float, [C.c_int, _fp]),
    "PvAmdBandwidthProbe": (C.c_int, [C.c_int, _fp]),
    "PvAmdSetEmitters": (C.c_int, [_vp, _fp, C.c_int]),
    "PvAmdGetOutput": (C.c_int, [_vp] + [C.c_float] * 3 + [C.POINTER(PlaneverbOutput)]),
    "PvAmdSetOutputQueries": (C.c_int, [_vp, _fp, C.c_int]),
    "PvAmdGetQueriedOutputs": (C.c_int, [_vp, C.POINTER(PlaneverbOutput), C.c_int]),
    "PvAmdSetQueryRecords": (C.c_int, [_vp, C.c_uint]),
    "PvAmdGetQueryRecordKinds": (C.c_uint, [_vp]),
    "PvAmdQueryRecordFloats": (C.c_int, [_vp, C.c_uint]),
    "PvAmdGetQueriedRecords": (C.c_int, [_vp, C.c_uint, _fp, C.c_int]),
    "PvAmdSetRecordQueries": (C.c_int, [_vp, _fp, C.c_int]),
    "PvAmdSetQuerySpectralRecords": (C.c_int, [_vp, C.c_uint]),
    "PvAmdGetQuerySpectralKinds": (C.c_uint, [_vp]),
    "PvAmdQuerySpectralFloats": (C.c_int, [_vp, C.c_uint]),
    "PvAmdGetQueriedSpectralRecords": (C.c_int, [_vp, C.c_uint, _fp, C.c_int]),
    "PvAmdSetEmitterRecords": (C.c_int, [_vp, C.c_uint, C.c_uint]),
    "PvAmdGetEmitterRecordKinds": (C.c_int, [_vp, C.POINTER(C.c_uint), C.POINTER(C.c_uint)]),
    "PvAmdEmitterRecordFloats": (C.c_int, [_vp, C.c_int, C.c_uint]),
    "PvAmdGetEmitterRecords": (C.c_int, [_vp, C.c_int, C.c_uint, _fp, C.c_int]),
    "PvAmdGetEmitterCells": (C.c_int, [_vp, C.POINTER(C.c_int), C.c_int]),
    "PvAmdCopyEmitterTrace": (C.c_int, [_vp, C.c_int, _fp]),
    "PvAmdCopyResults": (C.c_int, [_vp, _fp, _fp]),
    "PvAmdCopyResultsBlock": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _fp, _fp]),
    "PvAmdGetImpulseResponse": (C.c_int, [_vp, C.c_int, C.c_int, _fp]),
    "PvAmdGetImpulseResponseCells": (C.c_int, [_vp, C.c_int, C.c_int, C.POINTER(PlaneverbCell)]),
    "PvAmdCopyFields": (C.c_int, [_vp, _fp, _fp, _fp]),
    "PvAmdCopyHistoryPlane": (C.c_int, [_vp, C.c_int, _fp]),
    "PvAmdSetHistoryPlane": (C.c_int, [_vp, C.c_int, _fp]),
    "PvAmdLibmProbe": (C.c_int, [C.c_int, _fp, _fp, C.c_longlong, C.c_int]),
    "PvAmdComputeRoomMetrics": (C.c_int, [_vp, _fp]),
    "PvAmdCopyRoomMetrics": (C.c_int, [_vp, _fp]),
    "PvAmdCopyRoomMetricsBlock": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _fp]),
    "PvAmdGetRoomMetrics": (C.c_int, [_vp] + [C.c_float] * 3 + [C.POINTER(PvAmdRoomMetrics)]),
    "PvAmdHostRoomMetrics": (C.c_int, [_fp, C.c_int, C.c_int, C.c_int, C.POINTER(PvAmdRoomMetrics)]),
    "PvAmdComputeDecayTimes": (C.c_int, [_vp, _fp]),
    "PvAmdCopyDecayTimes": (C.c_int, [_vp, _fp]),
    "PvAmdCopyDecayTimesBlock": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _fp]),
    "PvAmdGetDecayTimes": (C.c_int, [_vp] + [C.c_float] * 3 + [C.POINTER(PvAmdDecayTimes)]),
    "PvAmdHostDecayTimes": (C.c_int, [_fp, C.c_int, C.c_int, C.c_int, C.POINTER(PvAmdDecayTimes)]),
    "PvAmdComputeEchoCriterion": (C.c_int, [_vp, _fp]),
    "PvAmdCopyEchoCriterion": (C.c_int, [_vp, _fp]),
    "PvAmdCopyEchoCriterionBlock": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _fp]),
    "PvAmdGetEchoCriterion": (C.c_int, [_vp] + [C.c_float] * 3 + [C.POINTER(PvAmdEchoCriterion)]),
    "PvAmdHostEchoCriterion": (C.c_int, [_fp, C.c_int, C.c_int, C.c_int, C.POINTER(PvAmdEchoCriterion)]),
    "PvAmdComputeLateralFraction": (C.c_int, [_vp, _fp]),
    "PvAmdCopyLateralFraction": (C.c_int, [_vp, _fp]),
    "PvAmdCopyLateralFractionBlock": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _fp]),
    "PvAmdGetLateralFraction": (C.c_int, [_vp] + [C.c_float] * 3 + [C.POINTER(PvAmdLateralFraction)]),
    "PvAmdHostLateralFraction": (C.c_int, [_fp, _fp, _fp, C.c_int, C.c_int, C.c_int, C.POINTER(PvAmdLateralFraction)]),
    "PvAmdSetEchogram": (C.c_int, [_vp, C.c_float, C.c_int]),
    "PvAmdGetEchogramSlots": (C.c_int, [_vp, _fp, C.POINTER(C.c_int)]),
    "PvAmdComputeEchogram": (C.c_int, [_vp, _fp]),
    "PvAmdCopyEchogram": (C.c_int, [_vp, _fp]),
    "PvAmdCopyEchogramBlock": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _fp]),
    "PvAmdGetEchogram": (C.c_int, [_vp] + [C.c_float] * 3 + [_fp]),
    "PvAmdHostEchogram": (C.c_int, [_fp, _fp, _fp, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, _fp]),
    "PvAmdSetLobeWindows": (C.c_int, [_vp, _fp, C.c_int]),
    "PvAmdGetLobeWindows": (C.c_int, [_vp, _fp, C.POINTER(C.c_int)]),
    "PvAmdComputeLobes": (C.c_int, [_vp, _fp]),
    "PvAmdCopyLobes": (C.c_int, [_vp, _fp]),
    "PvAmdCopyLobesBlock": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _fp]),
    "PvAmdGetLobes": (C.c_int, [_vp] + [C.c_float] * 3 + [_fp]),
    "PvAmdHostLobes": (C.c_int, [_fp, _fp, _fp, C.c_int, C.c_int, C.c_int, _fp, C.c_int, _fp]),
    "PvAmdLobeGains": (C.c_int, [_fp, C.c_int, C.c_float, C.c_float, C.c_int, _fp]),
    "PvAmdSetBands": (C.c_int, [_vp, _fp, C.c_int, C.c_int]),
    "PvAmdGetBands": (C.c_int, [_vp, _fp, C.c_int, C.POINTER(C.c_int)]),
    "PvAmdGetBandCoefs": (C.c_int, [_vp, _fp]),
    "PvAmdComputeBandMetrics": (C.c_int, [_vp, _fp]),
    "PvAmdCopyBandMetrics": (C.c_int, [_vp, _fp]),
    "PvAmdCopyBandMetricsBlock": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _fp]),
    "PvAmdGetBandMetrics": (C.c_int, [_vp] + [C.c_float] * 3 + [_fp]),
    "PvAmdHostBandCoefs": (C.c_int, [C.c_int, _fp, C.c_int, C.c_int, _fp]),
    "PvAmdHostBandMetrics": (C.c_int, [_fp, C.c_int, C.c_int, C.c_int, _fp, C.c_int, _fp]),
    "PvAmdSetModulationFrequencies": (C.c_int, [_vp, _fp]),
    "PvAmdGetModulationFrequencies": (C.c_int, [_vp, _fp]),
    "PvAmdComputeModulation": (C.c_int, [_vp, _fp]),
    "PvAmdCopyModulation": (C.c_int, [_vp, _fp]),
    "PvAmdCopyModulationBlock": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _fp]),
    "PvAmdGetModulation": (C.c_int, [_vp] + [C.c_float] * 3 + [_fp]),
    "PvAmdHostModulation": (C.c_int, [_fp, C.c_int, C.c_int, C.c_int, _fp, C.c_int, _fp, _fp]),
    "PvAmdHostModulationTable": (C.c_int, [C.c_int, C.c_int, _fp, _fp]),
    "PvAmdCombineMti": (C.c_int, [_fp, _fp, _fp, C.c_int, _fp]),
    "PvAmdSetSpectrumBins": (C.c_int, [_vp, _fp, C.c_int]),
    "PvAmdGetSpectrumBins": (C.c_int, [_vp, _fp, C.c_int]),
    "PvAmdGetSpectrumSource": (C.c_int, [_vp, _fp]),
    "PvAmdComputeSpectrum": (C.c_int, [_vp, _fp]),
    "PvAmdCopySpectrum": (C.c_int, [_vp, _fp]),
    "PvAmdCopySpectrumBlock": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _fp]),
    "PvAmdGetSpectrum": (C.c_int, [_vp] + [C.c_float] * 3 + [_fp]),
    "PvAmdHostSpectrumTables": (C.c_int, [C.c_int, C.c_int, _fp, C.c_int, _fp, _fp]),
    "PvAmdHostSpectrum": (C.c_int, [_fp, C.c_int, C.c_int, C.c_int, _fp, C.c_int, _fp, _fp]),
    "PvAmdSetWaterfall": (C.c_int, [_vp, _fp, C.c_int, C.c_float, C.c_int]),
    "PvAmdGetWaterfall": (C.c_int, [_vp, _fp, C.c_int, _fp, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "PvAmdWaterfallFloats": (C.c_int, [_vp]),
    "PvAmdComputeWaterfall": (C.c_int, [_vp, _fp, C.c_int, _fp]),
    "PvAmdCopyWaterfall": (C.c_int, [_vp, _fp, C.c_int]),
    "PvAmdHostWaterfall": (C.c_int, [_fp, C.c_int, C.c_int, C.c_int, _fp, C.c_int, C.c_float, C.c_int, _fp, _fp]),
    "PvAmdSetArrays": (C.c_int, [_vp, C.POINTER(C.c_int), C.c_int, _fp, C.c_int]),
    "PvAmdGetArrays": (C.c_int, [_vp, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int)]),
    "PvAmdGetArrayTaps": (C.c_int, [_vp, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), _fp, C.c_int]),
    "PvAmdSetArrayRecords": (C.c_int, [_vp, C.c_uint, C.c_uint]),
    "PvAmdGetArrayRecordKinds": (C.c_int, [_vp, C.POINTER(C.c_uint), C.POINTER(C.c_uint)]),
    "PvAmdArrayRecordFloats": (C.c_int, [_vp, C.c_int, C.c_uint]),
    "PvAmdComputeArrays": (C.c_int, [_vp, _fp]),
    "PvAmdCopyArrayResponse": (C.c_int, [_vp, C.c_int, _fp]),
    "PvAmdGetArrayOnsets": (C.c_int, [_vp, _fp, C.c_int]),
    "PvAmdGetArrayRecords": (C.c_int, [_vp, C.c_int, C.c_uint, _fp, C.c_int]),
    "PvAmdHostArrayTaps": (C.c_int, [C.c_int, C.c_int, C.c_float, C.c_float, C.c_int, C.POINTER(C.c_int), _fp]),
    "PvAmdHostArrayResponse": (C.c_int, [_fp, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), _fp, C.c_int, _fp, _fp]),
    "PvAmdSetAuralisation": (C.c_int, [_vp, C.c_int, C.c_int, C.c_float]),
    "PvAmdGetAuralisation": (C.c_int, [_vp, C.POINTER(C.c_int), C.POINTER(C.c_int), _fp, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "PvAmdGetAuralTaps": (C.c_int, [_vp, C.POINTER(C.c_int), _fp, C.c_int]),
    "PvAmdComputeAuralResponses": (C.c_int, [_vp, C.c_int, _fp, C.c_int, _fp]),
    "PvAmdCopyAuralResponse": (C.c_int, [_vp, C.c_int, _fp]),
    "PvAmdAuralise": (C.c_int, [_vp, _fp, C.c_int, C.c_int, C.POINTER(C.c_int), _fp, _fp]),
    "PvAmdCopyAuralOutput": (C.c_int, [_vp, C.c_int, _fp]),
    "PvAmdCopyAuralMix": (C.c_int, [_vp, _fp]),
    "PvAmdAuralShape": (None, [C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "PvAmdSetAuralForm": (C.c_int, [_vp, C.c_int]),
    "PvAmdHostAuralTaps": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.POINTER(C.c_int), _fp, C.c_int, C.POINTER(C.c_int),
                                     C.POINTER(C.c_int)]),
    "PvAmdHostAuralResample": (C.c_int, [_fp, C.c_int, C.POINTER(C.c_int), _fp, C.c_int, C.c_int, _fp]),
    "PvAmdHostAuralConvolve": (C.c_int, [_fp, C.c_int, _fp, C.c_int, _fp]),
    "PvAmdSetZones": (C.c_int, [_vp, C.POINTER(C.c_ubyte), C.c_int]),
    "PvAmdGetZones": (C.c_int, [_vp, C.POINTER(C.c_ubyte), C.POINTER(C.c_int)]),
    "PvAmdZoneStatPlanes": (C.c_int, [_vp, C.c_int]),
    "PvAmdComputeZoneStats": (C.c_int, [_vp, C.c_int, _vp, C.c_int, _fp]),
    "PvAmdHostZoneStats": (C.c_int, [_fp, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_ubyte), C.c_int, _vp]),
    "PvAmdHostZoneRects": (C.c_int, [C.c_float, C.c_int, C.c_int, _fp, C.c_int, C.POINTER(C.c_ubyte)]),
    "PvAmdComputeZoneDecay": (C.c_int, [_vp, C.c_int, _vp, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), _fp]),
    "PvAmdZoneDecayChunkSlots": (C.c_int, [_vp]),
    "PvAmdSetZoneCurves": (C.c_int, [_vp, C.c_int]),
    "PvAmdGetZoneCurves": (C.c_int, [_vp, C.POINTER(C.c_int)]),
    "PvAmdSetZoneMaps": (C.c_int, [_vp, C.c_uint]),
    "PvAmdGetZoneMaps": (C.c_int, [_vp, C.POINTER(C.c_uint)]),
    "PvAmdHostRoomSumsAdvance": (C.c_int, [_fp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _fp]),
    "PvAmdHostRoomMetricsFromSums": (C.c_int, [_fp, C.c_int, C.POINTER(PvAmdRoomMetrics)]),
    "PvAmdHostSpectrumAdvance": (C.c_int, [_fp, C.c_int, C.c_int, C.c_int, C.c_int, _fp, _fp, C.c_int, _fp]),
    "PvAmdHostZoneTiles": (C.c_int, [C.POINTER(C.c_ubyte)] + [C.c_int] * 4 + [C.POINTER(C.c_ubyte), C.POINTER(C.c_int)]),
    "PvAmdHostZoneTileUnion": (C.c_int, [C.POINTER(C.c_ubyte), C.POINTER(C.c_ubyte), C.c_int, C.POINTER(C.c_ubyte)]),
    "PvAmdHostZoneCurveChunk": (C.c_int, [C.c_int, C.c_int, C.c_longlong]),
    "PvAmdComputeZoneBandDecay": (C.c_int, [_vp, C.c_int, _vp, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), _fp]),
    "PvAmdZoneBandDecayChunk": (C.c_int, [_vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "PvAmdHostZoneBandDecay": (C.c_int, [_fp, _fp] + [C.c_int] * 4 + [C.POINTER(C.c_ubyte), C.c_int, _fp, C.c_int, C.c_int, _vp,
                                         C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "PvAmdHostZoneCurveClarity": (C.c_int, [C.POINTER(C.c_double), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double)]),
    "PvAmdHostZoneDecay": (C.c_int, [_fp, _fp] + [C.c_int] * 4 + [C.POINTER(C.c_ubyte), C.c_int, C.c_int, _vp, C.POINTER(C.c_double),
                                                                   C.POINTER(C.c_double)]),
    "PvAmdCopyPulse": (C.c_int, [_vp, _fp]),
    "PvAmdCopyMaterial": (C.c_int, [_vp, C.POINTER(C.c_ubyte), _fp]),
    "PvAmdSetFields": (C.c_int, [_vp, _fp, _fp, _fp]),
    "PvAmdRunSteps": (C.c_int, [_vp, C.c_int, C.c_int, C.c_float, C.c_float]),
    "PvAmdShardPlan": (C.c_int, [C.c_int] * 4 + [C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int]),
    "PvAmdPlanSegments": (C.c_int, [C.POINTER(C.c_ubyte)] + [C.c_int] * 5 + [C.POINTER(C.c_int), C.c_int]),
    "PvAmdCommUniqueId": (C.c_int, [C.c_char_p]),
    "PvAmdCommCreate": (_vp, [C.c_char_p, C.c_int, C.c_int, C.c_int]),
    "PvAmdCommDestroy": (None, [_vp]),
    "PvAmdCommAllGather": (C.c_int, [_vp, _fp, C.c_int, _fp]),
    "PvAmdRunSharded": (C.c_int, [C.POINTER(_vp), C.c_int, _fp, C.c_int, _fp, C.c_int, C.c_int, C.c_int, _vp,
                                  C.POINTER(PlaneverbOutput)]),
    "PvAmdReverbBusGains": (None, [C.c_float, C.c_float, _fp, _fp, _fp]),
    "PvAmdHostGridInfo": (C.c_int, [C.c_float, C.c_float, C.c_int, C.POINTER(PvAmdInfo)]),
    "PvAmdHostPulse": (C.c_int, [C.c_float, C.c_float, C.c_int, _fp]),
    "PvAmdHostPulseSelfCheck": (C.c_int, []),
    "PvAmdHostRasterize": (C.c_int, [C.c_float, C.c_float, C.c_int, _fp, C.POINTER(C.c_int), C.c_int,
                                     C.POINTER(C.c_ubyte), _fp]),
    "PvAmdHostLoadPv": (C.c_int, [C.c_char_p, _fp, C.c_int]),
    "PvAmdHostSavePv": (C.c_int, [C.c_char_p, _fp, C.POINTER(C.c_int), C.c_int]),
    "PvAmdHostCells": (C.c_int, [C.c_float, C.c_float, C.c_int, C.c_float, C.c_float] + [C.POINTER(C.c_int)] * 5),
    "PvAmdBakeCreate": (_vp, [_vp, C.c_int] + [C.c_float] * 4 + [C.c_int, C.c_int]),
    "PvAmdBakeRun": (C.c_int, [_vp, C.POINTER(_vp), C.c_int, C.c_int, C.c_int]),
    "PvAmdBakeMerge": (C.c_int, [_vp, _vp]),
    "PvAmdBakeSave": (C.c_int, [_vp, C.c_char_p]),
    "PvAmdBakeLoad": (_vp, [C.c_char_p]),
    "PvAmdBakeDestroy": (None, [_vp]),
    "PvAmdBakeGetInfo": (C.c_int, [_vp, C.POINTER(PvAmdBakeInfo)]),
    "PvAmdBakeProbe": (C.c_int, [_vp, C.c_int, C.POINTER(C.c_int), _fp]),
    "PvAmdBakeQuery": (C.c_int, [_vp, _fp, _fp, C.c_int, _fp]),
    "PvAmdBakeQueryDevice": (C.c_int, [_vp, C.c_int, _fp, _fp, C.c_int, _fp]),
}

_lib = None


def lib():
    """Load libplaneverb_amd.so (built by planeverb_amd.build.build()).  Raises if it is missing: there is no
    fallback implementation."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("%s not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                               "(hipcc --offload-arch=gfx950)" % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def variant(lib_path):
    """This module once more, bound to ANOTHER build of the library -- e.g. libplaneverb_amd_exp.so, the experimental build
    (make EXTRA=-DPV_EXPERIMENTAL) that carries the kernel arms and tile configurations the product library leaves out.
    Both libraries can be used side by side in one process (each has its own state)."""
    import importlib.util
    import sys
    name = "%s_variant_%s" % (__name__, os.path.splitext(os.path.basename(lib_path))[0])
    if name in sys.modules:
        return sys.modules[name]
    spec = importlib.util.spec_from_file_location(name, __file__)
    mod = importlib.util.module_from_spec(spec)
    mod.__package__ = __package__
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    mod.LIB_PATH = lib_path
    return mod


def last_error():
    e = lib().PvAmdLastError()
    return e.decode() if e else ""


class PlaneverbError(RuntimeError):
    pass


def _check(rc):
    if rc != 0:
        raise PlaneverbError(last_error())


def _f(a):
    return a.ctypes.data_as(_fp)


# --------------------------------------------------------------------------------------------------------------
# reference-shaped live API (Planeverb.h:12-47)
# --------------------------------------------------------------------------------------------------------------

Config = namedtuple("PlaneverbConfig", "gridSizeInMeters gridResolution gridBoundaryType tempFileDirectory "
                                       "maxThreadUsage threadExecutionType")
pv_CPU, pv_GPU = 0, 1  # PvTypes.h:13-17 / PlaneverbConfig.cs:23-29
pv_AbsorbingBoundary, pv_ReflectingBoundary = 0, 1  # gridBoundaryType, PvTypes.h:32-36 / PlaneverbConfig.cs:15-18


def Init(config):
    """Planeverb::Init (PvContext.cpp:25-32).  Raises PlaneverbError where the reference throws."""
    d = config.tempFileDirectory
    lib().PlaneverbInit(config.gridSizeInMeters[0], config.gridSizeInMeters[1], config.gridResolution,
                        config.gridBoundaryType, d.encode() if d is not None else None, config.maxThreadUsage,
                        config.threadExecutionType)
    if not lib().PlaneverbIsRunning():
        raise PlaneverbError(last_error() or "pv_InvalidConfig")


def Exit():
    lib().PlaneverbExit()


def Emit(pos):
    return lib().PlaneverbEmit(*[float(v) for v in pos])


def UpdateEmission(eid, pos):
    lib().PlaneverbUpdateEmission(int(eid), *[float(v) for v in pos])


def EndEmission(eid):
    lib().PlaneverbEndEmission(int(eid))


def GetOutput(eid):
    return lib().PlaneverbGetOutput(int(eid))


def AddGeometry(aabb):
    """aabb = (posX, posY, width, height, absorption), PvMathTypes.h:31-49"""
    return lib().PlaneverbAddGeometry(*[float(v) for v in aabb])


def UpdateGeometry(gid, aabb):
    lib().PlaneverbUpdateGeometry(int(gid), *[float(v) for v in aabb])


def RemoveGeometry(gid):
    lib().PlaneverbRemoveGeometry(int(gid))


def _xy(vertices):
    """vertex list [(x, y), ...] or flat [x0, y0, ...] -> (contiguous float32 array, n)"""
    a = np.ascontiguousarray(vertices, np.float32).reshape(-1)
    if a.size % 2:
        raise ValueError("vertex list with an odd number of coordinates")
    return a, a.size // 2


def AddOrientedGeometry(box):
    """box = (posX, posY, width, height, axisX, axisY, absorption): an oriented box (shape ids, not AABB ids); -1 if refused"""
    return lib().PlaneverbAddOrientedGeometry(*[float(v) for v in box])


def UpdateOrientedGeometry(sid, box):
    lib().PlaneverbUpdateOrientedGeometry(int(sid), *[float(v) for v in box])


def RemoveOrientedGeometry(sid):
    lib().PlaneverbRemoveOrientedGeometry(int(sid))


def AddPolygonGeometry(vertices, absorption):
    """a convex polygon of 3..8 vertices in grid metres (shape ids); -1 if refused"""
    a, n = _xy(vertices)
    return lib().PlaneverbAddPolygonGeometry(_f(a), n, float(absorption))


def UpdatePolygonGeometry(sid, vertices, absorption):
    a, n = _xy(vertices)
    lib().PlaneverbUpdatePolygonGeometry(int(sid), _f(a), n, float(absorption))


def RemovePolygonGeometry(sid):
    lib().PlaneverbRemovePolygonGeometry(int(sid))


def AddDiscGeometry(cx, cy, radius, absorption):
    """a disc in grid metres (shape ids); -1 if refused"""
    return lib().PlaneverbAddDiscGeometry(float(cx), float(cy), float(radius), float(absorption))


def UpdateDiscGeometry(sid, cx, cy, radius, absorption):
    lib().PlaneverbUpdateDiscGeometry(int(sid), float(cx), float(cy), float(radius), float(absorption))


def RemoveDiscGeometry(sid):
    lib().PlaneverbRemoveDiscGeometry(int(sid))


def AddWallPathGeometry(points, radius, absorption):
    """a polyline of 2..64 points with a radius (half the wall's thickness): one shape; -1 if refused"""
    a, n = _xy(points)
    return lib().PlaneverbAddWallPathGeometry(_f(a), n, float(radius), float(absorption))


def UpdateWallPathGeometry(sid, points, radius, absorption):
    a, n = _xy(points)
    lib().PlaneverbUpdateWallPathGeometry(int(sid), _f(a), n, float(radius), float(absorption))


def RemoveWallPathGeometry(sid):
    lib().PlaneverbRemoveWallPathGeometry(int(sid))


def AddConcavePolygonGeometry(vertices, absorption):
    """a simple polygon of 3..64 vertices, concave allowed, either winding (shape ids); -1 if refused"""
    a, n = _xy(vertices)
    return lib().PlaneverbAddConcavePolygonGeometry(_f(a), n, float(absorption))


def UpdateConcavePolygonGeometry(sid, vertices, absorption):
    a, n = _xy(vertices)
    lib().PlaneverbUpdateConcavePolygonGeometry(int(sid), _f(a), n, float(absorption))


def RemoveConcavePolygonGeometry(sid):
    lib().PlaneverbRemoveConcavePolygonGeometry(int(sid))


def AddMeshGeometry(vertices, triangles, absorption, mode=0, radius=0.0):
    """a triangle mesh (Solver.add_mesh), copied into the module's store at this call (mesh ids); -1 if refused"""
    v, t, tp = _mesh(vertices, triangles)
    return lib().PlaneverbAddMeshGeometry(_f(v), v.shape[0], tp, t.shape[0], float(absorption), int(mode), float(radius))


def SetMeshGeometryTransform(mid, transform):
    m, mp = _m12(transform)
    lib().PlaneverbSetMeshGeometryTransform(int(mid), mp)


def RemoveMeshGeometry(mid):
    lib().PlaneverbRemoveMeshGeometry(int(mid))


def SetSliceHeight(h):
    """the world height at which the meshes are sliced, applied at the next iteration boundary (pass the listener's y)"""
    lib().PlaneverbSetSliceHeight(float(h))


def SetGridBoundary(xmin, xmax, zmin, zmax):
    """absorption of the four grid edges (Solver.set_grid_boundary), applied at the next iteration boundary"""
    lib().PlaneverbSetGridBoundary(float(xmin), float(xmax), float(zmin), float(zmax))


def SetEdgeLayer(xmin, xmax, zmin, zmax):
    """widths in cells of the graded absorbing layers along the four grid edges (Solver.set_edge_layer), applied at the next
    iteration boundary; a refusal (sparse-emitter mode, widths the grid cannot hold) changes nothing and sets last_error()"""
    lib().PlaneverbSetEdgeLayer(int(xmin), int(xmax), int(zmin), int(zmax))


def SetEdgeLayerSplit(xmin, xmax, zmin, zmax):
    """SetEdgeLayer with the split-field model at EDGE_LAYER_SPLIT_R0 (Solver.set_edge_layer_split); SetEdgeLayer afterwards
    selects the unsplit model again"""
    lib().PlaneverbSetEdgeLayerSplit(int(xmin), int(xmax), int(zmin), int(zmax))


def SetListenerPosition(pos):
    lib().PlaneverbSetListenerPosition(*[float(v) for v in pos])


def GetImpulseResponse(pos):
    """Planeverb::GetImpulseResponse (Planeverb.h:47): structured array [T] of (pr, vx, vy, b, by) at a world position,
    from the last completed iteration; empty for a position outside the cell array"""
    n = lib().PlaneverbGetImpulseResponse(float(pos[0]), float(pos[1]), float(pos[2]), None, 0)
    if n < 0:
        raise PlaneverbError(last_error())
    out = np.zeros(n, CELL_DTYPE)
    if n:
        got = lib().PlaneverbGetImpulseResponse(float(pos[0]), float(pos[1]), float(pos[2]),
                                                out.ctypes.data_as(C.POINTER(PlaneverbCell)), n)
        if got != n:
            raise PlaneverbError(last_error())
    return out


def SetEmissionRecords(kinds):
    """the record kinds (a mask of QREC_*) every following iteration computes for the cells of the live emitters; 0 switches off"""
    _check(lib().PlaneverbSetEmissionRecords(int(kinds)))


def SetEmissionEchogram(slot_seconds, n_slots):
    _check(lib().PlaneverbSetEmissionEchogram(float(slot_seconds), int(n_slots)))


def SetEmissionLobeWindows(edges_seconds=None):
    """the lobe windows' edges in seconds; None or empty: the default windows"""
    e = np.ascontiguousarray([] if edges_seconds is None else edges_seconds, np.float32).reshape(-1)
    _check(lib().PlaneverbSetEmissionLobeWindows(_f(e) if len(e) else None, len(e)))


def EmissionRecordKinds():
    """the kinds the PUBLISHED iteration carries"""
    return int(lib().PlaneverbEmissionRecordKinds())


def EmissionRecordFloats(kind):
    """floats of ONE kind in the published iteration, -1 if it does not carry the kind"""
    return int(lib().PlaneverbEmissionRecordFloats(int(kind)))


def EmissionRecordCells():
    """distinct cells the published iteration served, -1 when the module is down"""
    return int(lib().PlaneverbEmissionRecordCells())


def GetEmissionRecord(eid, kind, capacity=None):
    """(ok, float32 array) of ONE kind for the emitter's current cell in the published iteration: ok = 1 the record, 0 quiet NaNs
    (ended or unknown id, off the map, a cell not in the iteration's table or without an onset), -1 nothing written (the array
    then keeps its fill of zeros; it is empty when the iteration does not carry the kind)"""
    n = EmissionRecordFloats(kind) if capacity is None else int(capacity)
    out = np.zeros(max(n, 0), np.float32)
    ok = lib().PlaneverbGetEmissionRecord(int(eid), int(kind), _f(out) if len(out) else None, len(out))
    return int(ok), out


def IsRunning():
    return bool(lib().PlaneverbIsRunning())


def LoadScene(path):
    n = lib().PlaneverbLoadScene(path.encode())
    if n < 0:
        raise PlaneverbError(last_error())
    return n


def WaitIterations(count, timeout_ms=60000):
    return lib().PlaneverbWaitIterations(int(count), int(timeout_ms))


def IterationCount():
    return lib().PlaneverbIterationCount()


def reverb_bus_gains(rt60, wet):
    a, b, c = C.c_float(), C.c_float(), C.c_float()
    lib().PvAmdReverbBusGains(rt60, wet, a, b, c)
    return a.value, b.value, c.value


def host_grid_info(size_x, size_y, res):
    i = PvAmdInfo()
    _check(lib().PvAmdHostGridInfo(float(size_x), float(size_y), int(res), i))
    return i


def host_pulse(size_x, size_y, res):
    i = host_grid_info(size_x, size_y, res)
    out = np.empty(i.T, np.float32)
    _check(lib().PvAmdHostPulse(float(size_x), float(size_y), int(res), _f(out)))
    return out


def host_rasterize(size_x, size_y, res, boxes, ops=None):
    i = host_grid_info(size_x, size_y, res)
    boxes = np.ascontiguousarray(boxes, np.float32).reshape(-1, 5)
    ops_a = np.ascontiguousarray(ops if ops is not None else np.ones(len(boxes)), np.int32)
    beta = np.empty((i.gx + 1, i.gy + 1), np.uint8)
    R = np.empty((i.gx + 1, i.gy + 1), np.float32)
    _check(lib().PvAmdHostRasterize(float(size_x), float(size_y), int(res), _f(boxes),
                                    ops_a.ctypes.data_as(C.POINTER(C.c_int)), len(boxes),
                                    beta.ctypes.data_as(C.POINTER(C.c_ubyte)), _f(R)))
    return beta, R


def host_oriented_box_vertices(px, py, w, h, ax, ay):
    """the 4 counter-clockwise vertices (4 x 2 float32) the library makes of an oriented box"""
    out = np.empty(8, np.float32)
    _check(lib().PvAmdHostOrientedBoxVertices(float(px), float(py), float(w), float(h), float(ax), float(ay), _f(out)))
    return out.reshape(4, 2)


def host_shape(vertices, absorption=0.0):
    """the shape the library makes of a vertex list: n x 2 float32, counter-clockwise (PlaneverbError if refused)"""
    a, n = _xy(vertices)
    out = np.empty(16, np.float32)
    m = lib().PvAmdHostShape(_f(a), n, float(absorption), _f(out))
    if m < 0:
        raise PlaneverbError(last_error())
    return out[:2 * m].reshape(m, 2)


SHAPE_DISC, SHAPE_CAPSULE, SHAPE_WALL_PATH, SHAPE_POLYGON = 1, 2, 3, 4
POLY_MAX_VERTS = 64


def host_coverage(size_x, size_y, res, kind, points, radius=0.0):
    """the cells (gx+1) x (gy+1) a disc / capsule / wall path / simple polygon covers on a grid of that configuration (uint8);
    kind = SHAPE_DISC (one point), SHAPE_CAPSULE (two), SHAPE_WALL_PATH or SHAPE_POLYGON; PlaneverbError if refused"""
    a, n = _xy(points)
    g = host_grid_info(size_x, size_y, res)
    cover = np.empty((g.gx + 1, g.gy + 1), np.uint8)
    _check(lib().PvAmdHostRoundShapeCoverage(float(size_x), float(size_y), int(res), int(kind), _f(a), n, float(radius),
                                             cover.ctypes.data_as(C.POINTER(C.c_ubyte))))
    return cover


MESH_SOLID, MESH_SHELL = 0, 1
MESH_MAX, MESH_MAX_TRIS, MESH_MAX_TRIS_TOTAL = 64, 1 << 20, 1 << 22


def _mesh(vertices, triangles):
    v = np.ascontiguousarray(vertices, np.float32)
    t = np.ascontiguousarray(triangles, np.int32)
    if v.ndim != 2 or v.shape[1] != 3 or t.ndim != 2 or t.shape[1] != 3:
        raise ValueError("a mesh is nv x 3 vertices (x, y, z) and nt x 3 triangle indices")
    return v, t, t.ctypes.data_as(C.POINTER(C.c_int))


def _m12(transform):
    if transform is None:
        return None, None
    m = np.ascontiguousarray(transform, np.float32).reshape(-1)
    if m.size != 12:
        raise ValueError("a mesh transform is 3 x 4, row-major")
    return m, _f(m)


def host_mesh_section(vertices, triangles, h=0.0, transform=None):
    """the section of every triangle at height h, as the library slices it: (segments nt x 4 float32 (a.x, a.z, b.x, b.z),
    valid nt uint8); transform: 3 x 4 row-major or None"""
    v, t, tp = _mesh(vertices, triangles)
    m, mp = _m12(transform)
    seg = np.empty((t.shape[0], 4), np.float32)
    valid = np.empty(t.shape[0], np.uint8)
    _check(lib().PvAmdHostMeshSection(_f(v), v.shape[0], tp, t.shape[0], mp, float(h), _f(seg),
                                      valid.ctypes.data_as(C.POINTER(C.c_ubyte))))
    return seg, valid


def host_mesh_coverage(size_x, size_y, res, vertices, triangles, h=0.0, mode=MESH_SOLID, radius=0.0, transform=None):
    """the cells (gx+1) x (gy+1) a mesh covers at slice height h on a grid of that configuration (uint8), on the CPU;
    PlaneverbError if the mesh is refused"""
    v, t, tp = _mesh(vertices, triangles)
    m, mp = _m12(transform)
    g = host_grid_info(size_x, size_y, res)
    cover = np.empty((g.gx + 1, g.gy + 1), np.uint8)
    _check(lib().PvAmdHostMeshCoverage(float(size_x), float(size_y), int(res), _f(v), v.shape[0], tp, t.shape[0], mp, float(h),
                                       int(mode), float(radius), cover.ctypes.data_as(C.POINTER(C.c_ubyte))))
    return cover


def host_shape_coverage(size_x, size_y, res, vertices):
    """the cells (gx+1) x (gy+1) the shape covers on a grid of that configuration (uint8)"""
    i = host_grid_info(size_x, size_y, res)
    a, n = _xy(vertices)
    cover = np.empty((i.gx + 1, i.gy + 1), np.uint8)
    _check(lib().PvAmdHostShapeCoverage(float(size_x), float(size_y), int(res), _f(a), n,
                                        cover.ctypes.data_as(C.POINTER(C.c_ubyte))))
    return cover


EDGE_LAYER_DEFAULT_WIDTH = 24  # cells: the width the edge-layer documentation and tests use (any 1..64 is accepted)
EDGE_LAYER_SPLIT_R0 = 1e-4  # PVA_EDGE_LAYER_SPLIT_R0: the split-field model's recommended design reflection


def _w4(w4):
    a = np.ascontiguousarray(w4, np.int32).reshape(-1)
    if a.size != 4:
        raise ValueError("four widths: x = 0, x = gx, y = 0, y = gy")
    return a


def edge_layer_tables(size_x, size_y, res, w4, r0=None):
    """the eight float32 damping tables of edge layers of widths w4 (PvAmdHostEdgeLayerTables, CPU only): a dict of apx, bpx,
    ax, bx (gx + 1 each) and apy, bpy, ay, by (gy + 1 each).  r0: the design reflection (PvAmdHostEdgeLayerTablesR0, the
    split model's tables); None = the unsplit model's tables"""
    i = host_grid_info(size_x, size_y, res)
    a = _w4(w4)
    out = np.empty(4 * (i.gx + 1) + 4 * (i.gy + 1), np.float32)
    wp = a.ctypes.data_as(C.POINTER(C.c_int))
    if r0 is None:
        n = lib().PvAmdHostEdgeLayerTables(float(size_x), float(size_y), int(res), wp, _f(out))
    else:
        n = lib().PvAmdHostEdgeLayerTablesR0(float(size_x), float(size_y), int(res), wp, float(r0), _f(out))
    if n < 0:
        raise PlaneverbError(last_error())
    nx, ny = i.gx + 1, i.gy + 1
    names = ["apx", "bpx", "ax", "bx", "apy", "bpy", "ay", "by"]
    offs = [0, nx, 2 * nx, 3 * nx, 4 * nx, 4 * nx + ny, 4 * nx + 2 * ny, 4 * nx + 3 * ny]
    return {k: out[o:o + (nx if j < 4 else ny)].copy() for j, (k, o) in enumerate(zip(names, offs))}


def host_enclosure(beta, seed, tile_rows=36, tile_cols=40, max_tiles=128):
    """PvAmdHostEnclosure: the air component of cell `seed` = (x, y) of beta[nx, ny] (non-zero = air) and the tile window around
    it, as a dict(found, cells, box=(r0, c0, r1, c1), window=(ti0, tj0, tis, tjs)); found = 0 when the seed is no air cell or the
    window would hold more than max_tiles tiles"""
    b = np.ascontiguousarray(beta, np.uint8)
    out = np.zeros(10, np.int32)
    if lib().PvAmdHostEnclosure(b.ctypes.data_as(C.POINTER(C.c_ubyte)), b.shape[0], b.shape[1], int(seed[0]), int(seed[1]),
                                int(tile_rows), int(tile_cols), int(max_tiles), out.ctypes.data_as(C.POINTER(C.c_int))) < 0:
        raise PlaneverbError(last_error())
    v = [int(x) for x in out]
    return dict(found=v[0], cells=v[1], box=tuple(v[2:6]), window=tuple(v[6:10]))


def host_window_clear(window_run, win, prev_rect, planes_dirty, swept_dirty, split_planes):
    """PvAmdHostWindowClear: what a run clears in front of its first launch -- 0 nothing, 1 the previous run's tile rectangle, 2 all
    planes; win, prev_rect = (first tile row, tile rows, first tile column, tile columns)"""
    w, p = ((C.c_int * 4)(*[int(v) for v in r]) for r in (win, prev_rect))
    rc = lib().PvAmdHostWindowClear(int(bool(window_run)), w, p, int(bool(planes_dirty)), int(bool(swept_dirty)), int(bool(split_planes)))
    if rc < 0:
        raise PlaneverbError(last_error())
    return rc


def load_pv(path, max_boxes=4096):
    """.pv scene -> (n, 5) float32 array of (posX, posY, width, height, absorption)"""
    buf = np.empty((max_boxes, 5), np.float32)
    n = lib().PvAmdHostLoadPv(path.encode(), _f(buf), max_boxes)
    if n < 0:
        raise PlaneverbError(last_error())
    return buf[:n].copy()


def save_pv(path, boxes, ids=None):
    """write boxes [(posX, posY, width, height, absorption), ...] as a .pv scene (Editor.cpp:219-243)"""
    b = np.ascontiguousarray(boxes, np.float32).reshape(-1, 5)
    ida = None if ids is None else np.ascontiguousarray(ids, np.int32)
    _check(lib().PvAmdHostSavePv(path.encode(), _f(b), None if ida is None else ida.ctypes.data_as(C.POINTER(C.c_int)),
                                 len(b)))


def host_room_metrics(p, fs, onset):
    """PvAmdHostRoomMetrics: float32 [10] (ROOM_METRIC_NAMES) of one impulse response p[T] with its onset step -- the
    definition of include/planeverb_amd.h (PvAmdRoomMetrics) on the CPU"""
    a = np.ascontiguousarray(p, np.float32).reshape(-1)
    out = PvAmdRoomMetrics()
    _check(lib().PvAmdHostRoomMetrics(_f(a) if a.size else None, int(a.size), int(fs), int(onset), out))
    return out.as_array()


def host_decay_times(p, fs, onset):
    """PvAmdHostDecayTimes: float32 [8] (DECAY_TIME_NAMES) of one impulse response p[T] with its onset step -- the
    definition of include/planeverb_amd.h (PvAmdDecayTimes) on the CPU"""
    a = np.ascontiguousarray(p, np.float32).reshape(-1)
    out = PvAmdDecayTimes()
    _check(lib().PvAmdHostDecayTimes(_f(a) if a.size else None, int(a.size), int(fs), int(onset), out))
    return out.as_array()


def host_echo_criterion(p, fs, onset):
    """PvAmdHostEchoCriterion: float32 [10] (ECHO_CRITERION_NAMES) of one impulse response p[T] with its onset step -- the
    definition of include/planeverb_amd.h (PvAmdEchoCriterion) on the CPU"""
    a = np.ascontiguousarray(p, np.float32).reshape(-1)
    out = PvAmdEchoCriterion()
    _check(lib().PvAmdHostEchoCriterion(_f(a) if a.size else None, int(a.size), int(fs), int(onset), out))
    return out.as_array()


def host_lateral_fraction(p, vx, vy, fs, onset):
    """PvAmdHostLateralFraction: float32 [11] (LATERAL_FRACTION_NAMES) of one impulse response p[T] with its velocities vx[T],
    vy[T] and its onset step -- the definition of include/planeverb_amd.h (PvAmdLateralFraction) on the CPU"""
    a, x, y = (np.ascontiguousarray(v, np.float32).reshape(-1) for v in (p, vx, vy))
    if not (a.size == x.size == y.size):
        raise ValueError("host_lateral_fraction: p, vx and vy must have the same length")
    out = PvAmdLateralFraction()
    ptr = [_f(v) if v.size else None for v in (a, x, y)]
    _check(lib().PvAmdHostLateralFraction(ptr[0], ptr[1], ptr[2], int(a.size), int(fs), int(onset), out))
    return out.as_array()


ECHOGRAM_MAX_SLOTS = 32  # PVA_ECHOGRAM_MAX_SLOTS


def host_echogram(p, vx, vy, fs, onset, slot_seconds, n_slots):
    """PvAmdHostEchogram: float32 [1 + 3 n_slots] (n, then e, ix, iy per slot) of one impulse response p[T] with its velocities
    vx[T], vy[T] and its onset step -- the definition of include/planeverb_amd.h (PvAmdSetEchogram) on the CPU"""
    a, x, y = (np.ascontiguousarray(v, np.float32).reshape(-1) for v in (p, vx, vy))
    if not (a.size == x.size == y.size):
        raise ValueError("host_echogram: p, vx and vy must have the same length")
    out = np.empty(1 + 3 * max(int(n_slots), 0), np.float32)
    ptr = [_f(v) if v.size else None for v in (a, x, y)]
    _check(lib().PvAmdHostEchogram(ptr[0], ptr[1], ptr[2], int(a.size), int(fs), int(onset), float(slot_seconds), int(n_slots),
                                   _f(out)))
    return out


LOBES_MAX_EDGES = 7  # PVA_LOBES_MAX_EDGES
# PVA_QREC_*: the record kinds Solver.set_query_records selects (a mask)
QREC_ROOM_METRICS = 1
QREC_DECAY_TIMES = 2
QREC_LATERAL = 4
QREC_ECHOGRAM = 8
QREC_ECHO_CRITERION = 16
QREC_LOBES = 32
QREC_ALL = 63
RECORD_QUERIES_MAX = 1024  # PVA_RECORD_QUERIES_MAX
# PVA_QSPEC_*: the in-run frequency-resolved record kinds (Solver.set_query_spectral_records), a selector of their own
QSPEC_BAND_METRICS = 1
QSPEC_MODULATION = 2
QSPEC_SPECTRUM = 4
QSPEC_ALL = 7
LOBES_DEFAULT_EDGES = (0.01, 0.08)
LOBE_NAMES = ("e", "xp", "xn", "yp", "yn")
LOBE_PATTERN_OMNI, LOBE_PATTERN_CARDIOID = 0, 1


def _lobe_edges(edges):
    e = np.ascontiguousarray(() if edges is None else edges, np.float32).reshape(-1)
    return e, (_f(e) if e.size else None)


def host_lobes(p, vx, vy, fs, onset, edges=None):
    """PvAmdHostLobes: float32 [1 + 5 nW] (n, then LOBE_NAMES per window) of one impulse response p[T] with its velocities vx[T],
    vy[T] and its onset step, for the window edges given in seconds (None or empty: the default, 10 ms and 80 ms) -- the
    definition of include/planeverb_amd.h (PvAmdSetLobeWindows) on the CPU"""
    a, x, y = (np.ascontiguousarray(v, np.float32).reshape(-1) for v in (p, vx, vy))
    if not (a.size == x.size == y.size):
        raise ValueError("host_lobes: p, vx and vy must have the same length")
    e, ep = _lobe_edges(edges)
    out = np.empty(1 + 5 * ((e.size or 2) + 1), np.float32)
    ptr = [_f(v) if v.size else None for v in (a, x, y)]
    _check(lib().PvAmdHostLobes(ptr[0], ptr[1], ptr[2], int(a.size), int(fs), int(onset), ep, int(e.size), _f(out)))
    return out


def lobe_gains(record, forward, pattern=LOBE_PATTERN_CARDIOID):
    """PvAmdLobeGains: float32 [nW], the energy ratio by which an emitter with the directivity `pattern` (0 omni, 1 cardioid)
    facing `forward` = (x, z), used as given, changes each window of the lobe record [1 + 5 nW] of its cell"""
    r = np.ascontiguousarray(record, np.float32).reshape(-1)
    if r.size < 6 or (r.size - 1) % 5:
        raise ValueError("lobe_gains: a record of 1 + 5 nW floats")
    nw = (r.size - 1) // 5
    out = np.empty(nw, np.float32)
    _check(lib().PvAmdLobeGains(_f(r), nw, float(forward[0]), float(forward[1]), int(pattern), _f(out)))
    return out


BANDS_MAX = 8  # PVA_BANDS_MAX
BAND_METRIC_NAMES = ("edt", "t20", "t30", "n_edt", "n_t20", "n_t30", "e0", "depth", "c50", "c80", "d50", "ts")


def host_band_coefs(fs, hz, fraction=1):
    """PvAmdHostBandCoefs: float32 [n, 10] (b0, b1, b2, a1, a2 of section 1, then of section 2) of the octave (fraction 1) or
    third-octave (fraction 3) Butterworth band-passes centred at hz for the sampling rate fs -- the design of
    include/planeverb_amd.h (PvAmdBandMetrics), in double on the CPU, rounded to float32 once"""
    h = np.ascontiguousarray(hz, np.float32).reshape(-1)
    out = np.empty((h.size, 10), np.float32)
    _check(lib().PvAmdHostBandCoefs(int(fs), _f(h) if h.size else None, int(h.size), int(fraction), _f(out)))
    return out


def host_band_metrics(p, fs, onset, coefs):
    """PvAmdHostBandMetrics: float32 [n, 12] (BAND_METRIC_NAMES) of one impulse response p[T] with its onset step, filtered
    backwards in time through the n coefficient sets coefs[n, 10] -- the definition of include/planeverb_amd.h on the CPU"""
    a = np.ascontiguousarray(p, np.float32).reshape(-1)
    c = np.ascontiguousarray(coefs, np.float32).reshape(-1, 10)
    out = np.empty((c.shape[0], 12), np.float32)
    _check(lib().PvAmdHostBandMetrics(_f(a) if a.size else None, int(a.size), int(fs), int(onset), _f(c) if c.size else None,
                                      int(c.shape[0]), _f(out)))
    return out


MODULATION_FREQS = 14  # PVA_MODULATION_FREQS
MODULATION_DEFAULT_HZ = (0.63, 0.8, 1.0, 1.25, 1.6, 2.0, 2.5, 3.15, 4.0, 5.0, 6.3, 8.0, 10.0, 12.5)  # IEC 60268-16


def _hz14(hz):
    if hz is None:
        return None
    h = np.ascontiguousarray(hz, np.float32).reshape(-1)
    if h.size != MODULATION_FREQS:
        raise ValueError("modulation: %d modulation frequencies, or None for the default" % MODULATION_FREQS)
    return h


def host_modulation_table(T, fs, hz=None):
    """PvAmdHostModulationTable: float32 [T, 14, 2] -- (cos, sin) of every modulation frequency hz (None: the default series) at
    every absolute step, computed in double on the CPU"""
    h = _hz14(hz)
    out = np.empty((max(int(T), 0), MODULATION_FREQS, 2), np.float32)
    _check(lib().PvAmdHostModulationTable(int(T), int(fs), _f(h) if h is not None else None, _f(out)))
    return out


def host_modulation(p, fs, onset, coefs, hz=None):
    """PvAmdHostModulation: float32 [n, 15] (m at the 14 modulation frequencies hz -- None: the default series -- then the band's
    modulation transfer index) of one impulse response p[T] with its onset step, filtered backwards in time through the n
    coefficient sets coefs[n, 10] -- the definition of include/planeverb_amd.h (PvAmdModulation) on the CPU"""
    a = np.ascontiguousarray(p, np.float32).reshape(-1)
    c = np.ascontiguousarray(coefs, np.float32).reshape(-1, 10)
    h = _hz14(hz)
    out = np.empty((c.shape[0], MODULATION_FREQS + 1), np.float32)
    _check(lib().PvAmdHostModulation(_f(a) if a.size else None, int(a.size), int(fs), int(onset), _f(c) if c.size else None,
                                     int(c.shape[0]), _f(h) if h is not None else None, _f(out)))
    return out


def combine_mti(mti, alpha, beta=()):
    """PvAmdCombineMti: sum(alpha[k] mti[k]) - sum(beta[k] sqrt(mti[k] mti[k + 1])) in float32, clamped to [0, 1]: the per-band
    modulation transfer indices of n adjacent bands combined with the caller's IEC 60268-16 weights (n alpha, n - 1 beta).  Over
    fewer than the seven octaves 125 Hz .. 8 kHz this is a partial index, not an STI"""
    m = np.ascontiguousarray(mti, np.float32).reshape(-1)
    a = np.ascontiguousarray(alpha, np.float32).reshape(-1)
    b = np.ascontiguousarray(beta, np.float32).reshape(-1)
    if a.size != m.size or b.size != max(m.size - 1, 0):
        raise ValueError("combine_mti: n indices, n weights alpha and n - 1 weights beta")
    out = C.c_float(0.0)
    _check(lib().PvAmdCombineMti(_f(m) if m.size else None, _f(a) if a.size else None, _f(b) if b.size else None, int(m.size),
                                 C.byref(out)))
    return np.float32(out.value)


SPECTRUM_MAX_BINS = 32  # PVA_SPECTRUM_MAX_BINS


def host_spectrum_tables(T, fs, hz):
    """PvAmdHostSpectrumTables: the twiddle tables (cos, sin), float32 [T, n] each, of the spectrum definition of
    include/planeverb_amd.h for the bins hz -- absolute run time, computed in double on the CPU"""
    h = np.ascontiguousarray(hz, np.float32).reshape(-1)
    c = np.empty((max(int(T), 0), h.size), np.float32)
    s = np.empty_like(c)
    _check(lib().PvAmdHostSpectrumTables(int(T), int(fs), _f(h) if h.size else None, int(h.size), _f(c), _f(s)))
    return c, s


def host_spectrum(p, fs, onset, hz, pulse):
    """PvAmdHostSpectrum: float32 [n, 3] (re, im, level in dB) of one impulse response p[T] with its onset step and the
    pulse table pulse[T] -- the spectrum definition of include/planeverb_amd.h on the CPU"""
    a = np.ascontiguousarray(p, np.float32).reshape(-1)
    q = np.ascontiguousarray(pulse, np.float32).reshape(-1)
    h = np.ascontiguousarray(hz, np.float32).reshape(-1)
    if q.size != a.size:
        raise ValueError("the pulse table and the impulse response differ in length")
    out = np.empty((h.size, 3), np.float32)
    _check(lib().PvAmdHostSpectrum(_f(a) if a.size else None, int(a.size), int(fs), int(onset), _f(h) if h.size else None,
                                   int(h.size), _f(q) if q.size else None, _f(out)))
    return out


WATERFALL_MAX_BINS = 512       # PVA_WATERFALL_MAX_BINS
WATERFALL_MAX_SLICES = 64      # PVA_WATERFALL_MAX_SLICES
WATERFALL_MAX_RECEIVERS = 256  # PVA_WATERFALL_MAX_RECEIVERS


def _waterfall_dict(rec, n, m):
    """records [N, 2 + 2 n + m n] as the parts of the Waterfall section of include/planeverb_amd.h"""
    N = rec.shape[0]
    return {"onset": rec[:, 0].copy(), "slices": rec[:, 1].copy(),
            "response": np.stack([rec[:, 2:2 + n], rec[:, 2 + n:2 + 2 * n]], axis=-1),
            "level": rec[:, 2 + 2 * n:].reshape(N, m, n).copy()}


def host_waterfall(p, fs, onset, hz, slice_seconds, n_slices, pulse):
    """PvAmdHostWaterfall: the record of one impulse response p[T] with its onset step and the pulse table pulse[T] -- the
    waterfall definition of include/planeverb_amd.h on the CPU -- as the dict Solver.waterfall returns for N = 1: onset [1],
    slices [1], response [1, n, 2] (R, I of slice 0), level [1, m, n] (dB re the source)"""
    a = np.ascontiguousarray(p, np.float32).reshape(-1)
    q = np.ascontiguousarray(pulse, np.float32).reshape(-1)
    h = np.ascontiguousarray(hz, np.float32).reshape(-1)
    if q.size != a.size:
        raise ValueError("the pulse table and the impulse response differ in length")
    n, m = int(h.size), int(n_slices)
    out = np.empty((1, 2 + 2 * n + max(m, 0) * n), np.float32)
    _check(lib().PvAmdHostWaterfall(_f(a) if a.size else None, int(a.size), int(fs), int(onset), _f(h) if h.size else None, n,
                                    float(slice_seconds), m, _f(q) if q.size else None, _f(out)))
    return _waterfall_dict(out, n, m)


ARRAYS_MAX = 256         # PVA_ARRAYS_MAX
ARRAY_MEMBERS_MAX = 64   # PVA_ARRAY_MEMBERS_MAX
ARRAY_NEAREST, ARRAY_LAGRANGE3 = 0, 1  # PVA_ARRAY_*: how a member's delay becomes taps


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


def host_array_taps(fs, T, gain, delay_seconds, interp=ARRAY_LAGRANGE3):
    """PvAmdHostArrayTaps: the taps of one array member (include/planeverb_amd.h, Source arrays) as (delays int32 [n], weights
    float32 [n]), n = 1 or 4; raises where the member is refused"""
    d, w = np.zeros(4, np.int32), np.zeros(4, np.float32)
    n = lib().PvAmdHostArrayTaps(int(fs), int(T), float(gain), float(delay_seconds), int(interp), _ip(d), _f(w))
    if n < 0:
        raise PlaneverbError(last_error())
    return d[:n].copy(), w[:n].copy()


def host_array_response(p, tap_member, tap_delay, tap_weight):
    """PvAmdHostArrayResponse: the response of one array from its members' responses p[M, T] and its taps in order, as
    (y float32 [T], onset float32 -- FLT_MAX: none)"""
    a = np.ascontiguousarray(p, np.float32)
    a = a.reshape(1, -1) if a.ndim == 1 else a
    m, d = np.ascontiguousarray(tap_member, np.int32).reshape(-1), np.ascontiguousarray(tap_delay, np.int32).reshape(-1)
    w = np.ascontiguousarray(tap_weight, np.float32).reshape(-1)
    if not (m.size == d.size == w.size):
        raise ValueError("the three tap lists differ in length")
    out, onset = np.empty(a.shape[1], np.float32), C.c_float(0.0)
    _check(lib().PvAmdHostArrayResponse(_f(a) if a.size else None, int(a.shape[0]), int(a.shape[1]), _ip(m) if m.size else None,
                                        _ip(d) if d.size else None, _f(w) if w.size else None, int(m.size), _f(out), C.byref(onset)))
    return out, np.float32(onset.value)


AURAL_MAX_TAPS = 1024        # PVA_AURAL_MAX_TAPS
AURAL_MAX_RECEIVERS = 256    # PVA_AURAL_MAX_RECEIVERS
AURAL_MAX_SIGNALS = 64       # PVA_AURAL_MAX_SIGNALS
AURAL_MAX_SAMPLES = 1 << 20  # PVA_AURAL_MAX_SAMPLES
AURAL_RECEIVERS, AURAL_ARRAYS = 0, 1  # PVA_AURAL_*: whose responses Solver.compute_aural_responses resamples
AURAL_TILED, AURAL_PLAIN = 0, 1       # PVA_AURAL_*: the convolution kernel Solver.auralise launches


def aural_shape():
    """PvAmdAuralShape: (outputs per block, taps per chunk) of the convolution kernel's tiling"""
    b, c = C.c_int(0), C.c_int(0)
    lib().PvAmdAuralShape(C.byref(b), C.byref(c))
    return b.value, c.value


def host_aural_shape(fs, T, rate, zero_crossings=16, beta=9.0):
    """(L, K) of a setting: the response length in output samples and the taps per sample; raises where it is refused"""
    L, K = C.c_int(0), C.c_int(0)
    _check(lib().PvAmdHostAuralTaps(int(fs), int(T), int(rate), int(zero_crossings), float(beta), None, None, 0, C.byref(L), C.byref(K)))
    return L.value, K.value


def host_aural_taps(fs, T, rate, zero_crossings=16, beta=9.0):
    """PvAmdHostAuralTaps: the resampling tables of a setting (include/planeverb_amd.h, Auralisation) as (first int32 [L], w
    float32 [L, K]); raises where the setting is refused"""
    L, K = host_aural_shape(fs, T, rate, zero_crossings, beta)
    first, w = np.empty(L, np.int32), np.empty((L, K), np.float32)
    _check(lib().PvAmdHostAuralTaps(int(fs), int(T), int(rate), int(zero_crossings), float(beta), _ip(first), _f(w), L, None, None))
    return first, w


def host_aural_resample(p, first, w):
    """PvAmdHostAuralResample: one response float32 [L] from samples p[T] and the tables (first [L], w [L, K])"""
    a = np.ascontiguousarray(p, np.float32).reshape(-1)
    f = np.ascontiguousarray(first, np.int32).reshape(-1)
    ww = np.ascontiguousarray(w, np.float32).reshape(f.size, -1)
    out = np.empty(f.size, np.float32)
    _check(lib().PvAmdHostAuralResample(_f(a) if a.size else None, int(a.size), _ip(f) if f.size else None, _f(ww) if ww.size else None,
                                        int(f.size), int(ww.shape[1]), _f(out)))
    return out


def host_aural_convolve(h, x):
    """PvAmdHostAuralConvolve: one output float32 [N + L - 1] from a response h[L] and a signal x[N]"""
    a = np.ascontiguousarray(h, np.float32).reshape(-1)
    b = np.ascontiguousarray(x, np.float32).reshape(-1)
    out = np.empty(max(a.size + b.size - 1, 1), np.float32)
    _check(lib().PvAmdHostAuralConvolve(_f(a) if a.size else None, int(a.size), _f(b) if b.size else None, int(b.size), _f(out)))
    return out


ZMAP_ROOM_METRICS, ZMAP_SPECTRUM = 1, 2  # PVA_ZMAP_*: the map kinds of Solver.set_zone_maps


def host_room_sums_advance(p, fs, onset, tA, tB, sums6=None):
    """PvAmdHostRoomSumsAdvance: the six room-metric sums (e50, l50, e80, l80, total, moment) of p[T] advanced over the accumulate
    pass [tA, tB) -- from +0.0 where the onset lies in the pass, else from sums6; float32 [6]"""
    a = np.ascontiguousarray(p, np.float32).reshape(-1)
    s = np.zeros(6, np.float32) if sums6 is None else np.array(sums6, np.float32).reshape(6)
    _check(lib().PvAmdHostRoomSumsAdvance(_f(a) if a.size else None, int(a.size), int(fs), int(onset), int(tA), int(tB), _f(s)))
    return s


def host_room_metrics_from_sums(sums6, fs):
    """PvAmdHostRoomMetricsFromSums: float32 [10] (ROOM_METRIC_NAMES) of six such sums"""
    s = np.ascontiguousarray(sums6, np.float32).reshape(6)
    out = PvAmdRoomMetrics()
    _check(lib().PvAmdHostRoomMetricsFromSums(_f(s), int(fs), out))
    return out.as_array()


def host_spectrum_advance(p, onset, tA, tB, cos_tn, sin_tn, reim=None):
    """PvAmdHostSpectrumAdvance: re, im of every bin (float32 [n, 2]) of p[T] advanced over the accumulate pass [tA, tB) with the
    tables of host_spectrum_tables -- from +0.0 where the onset lies in the pass, else from reim"""
    a = np.ascontiguousarray(p, np.float32).reshape(-1)
    c = np.ascontiguousarray(cos_tn, np.float32)
    s = np.ascontiguousarray(sin_tn, np.float32)
    if c.ndim != 2 or c.shape != s.shape or c.shape[0] != a.size:
        raise ValueError("host_spectrum_advance: tables [T, n]")
    n = c.shape[1]
    r = np.zeros((n, 2), np.float32) if reim is None else np.array(reim, np.float32).reshape(n, 2)
    _check(lib().PvAmdHostSpectrumAdvance(_f(a) if a.size else None, int(a.size), int(onset), int(tA), int(tB), _f(c), _f(s), int(n), _f(r)))
    return r


# PVA_MAP_*: the nine per-cell analysis kinds, as Solver.zone_stats names them (the stems of Solver.compute_<name> / <name>)
PVA_MAP_ROOM_METRICS, PVA_MAP_DECAY_TIMES, PVA_MAP_LATERAL_FRACTION, PVA_MAP_ECHO_CRITERION, PVA_MAP_ECHOGRAM = 0, 1, 2, 3, 4
PVA_MAP_LOBES, PVA_MAP_BAND_METRICS, PVA_MAP_MODULATION, PVA_MAP_SPECTRUM = 5, 6, 7, 8
MAP_KIND_NAMES = ("room_metrics", "decay_times", "lateral_fraction", "echo_criterion", "echogram", "lobes", "band_metrics",
                  "modulation", "spectrum")
ZONES_MAX = 64  # PVA_ZONES_MAX
# PvAmdZoneStat (64 bytes)
ZONE_STAT_DTYPE = np.dtype([("sum", "<f8"), ("mean", "<f8"), ("m2", "<f8"), ("std", "<f8"), ("min", "<f4"), ("max", "<f4"),
                            ("argmin", "<i4"), ("argmax", "<i4"), ("n_finite", "<i4"), ("n_nan", "<i4"), ("n_posinf", "<i4"),
                            ("n_neginf", "<i4")])
assert ZONE_STAT_DTYPE.itemsize == 64


def _map_kind(kind):
    if isinstance(kind, str):
        if kind not in MAP_KIND_NAMES:
            raise ValueError("zone statistics: kind is one of %s" % ", ".join(MAP_KIND_NAMES))
        return MAP_KIND_NAMES.index(kind)
    return int(kind)


def _zone_labels(labels, n_zones):
    lab = np.ascontiguousarray(labels, np.uint8)
    n = int(lab.max()) if n_zones is None and lab.size else int(n_zones or 0)
    return lab, n


def host_zone_stats(map, labels, n_zones=None):
    """PvAmdHostZoneStats: the zone statistics of include/planeverb_amd.h (PvAmdZoneStat) on the CPU -- map = float32
    [gx, gy, *width] as Solver.<kind>() returns it, labels = uint8 [gx, gy] (0: no zone, 1 .. n_zones; n_zones None: the largest
    label); a structured array (ZONE_STAT_DTYPE) of shape [n_zones, *width]"""
    m = np.ascontiguousarray(map, np.float32)
    lab, n = _zone_labels(labels, n_zones)
    if m.ndim < 2 or lab.shape != m.shape[:2]:
        raise ValueError("host_zone_stats: a map [gx, gy, ...] and labels [gx, gy]")
    width = m.shape[2:]
    planes = int(np.prod(width, dtype=np.int64))
    out = np.zeros((max(n, 0), planes), ZONE_STAT_DTYPE)
    _check(lib().PvAmdHostZoneStats(_f(m) if m.size else None, m.shape[0], m.shape[1], planes,
                                    lab.ctypes.data_as(C.POINTER(C.c_ubyte)), n, out.ctypes.data_as(_vp)))
    return out.reshape((n,) + width)


def zone_labels_from_rects(dx, gx, gy, rects):
    """PvAmdHostZoneRects: uint8 [gx, gy] -- cell (X, Y) gets j + 1 where rects[j] = (xmin, zmin, xmax, zmax) in metres holds
    its centre ((X + 0.5) dx, (Y + 0.5) dx), float32, half-open; later rectangles overwrite earlier ones; 0 elsewhere"""
    r = np.ascontiguousarray(rects, np.float32).reshape(-1, 4)
    out = np.zeros((int(gx), int(gy)), np.uint8)
    _check(lib().PvAmdHostZoneRects(float(dx), int(gx), int(gy), _f(r) if r.size else None, len(r),
                                    out.ctypes.data_as(C.POINTER(C.c_ubyte))))
    return out


def host_zone_tiles(labels, tile_rows, tile_cols):
    """PvAmdHostZoneTiles: (flags uint8 [ceil(gx / tile_rows), ceil(gy / tile_cols)], (row0, row1, blk0, blk1)) -- the tiles that
    hold a labelled cell and the labels' bounding box in result rows and blocks of 64 Y ((0, -1, 0, -1): nothing labelled); what
    Solver.set_zone_curves derives from the labels"""
    lab = np.ascontiguousarray(labels, np.uint8)
    if lab.ndim != 2 or not lab.size:
        raise ValueError("host_zone_tiles: labels [gx, gy]")
    gx, gy = lab.shape
    flags = np.zeros((-(-gx // int(tile_rows)), -(-gy // int(tile_cols))), np.uint8)
    box = (C.c_int * 4)()
    _check(lib().PvAmdHostZoneTiles(lab.ctypes.data_as(C.POINTER(C.c_ubyte)), gx, gy, int(tile_rows), int(tile_cols),
                                    flags.ctypes.data_as(C.POINTER(C.c_ubyte)), box))
    return flags, tuple(box)


def host_zone_tile_union(emitter_flags, zone_flags, n_tiles):
    """PvAmdHostZoneTileUnion: uint8 [n_tiles], 1 where either side (uint8 [n_tiles], or None) is set"""
    sides = [None if f is None else np.ascontiguousarray(f, np.uint8).reshape(-1) for f in (emitter_flags, zone_flags)]
    if any(f is not None and f.size != int(n_tiles) for f in sides):
        raise ValueError("host_zone_tile_union: flags of n_tiles bytes")
    out = np.zeros(int(n_tiles), np.uint8)
    _check(lib().PvAmdHostZoneTileUnion(*[None if f is None else f.ctypes.data_as(C.POINTER(C.c_ubyte)) for f in sides], int(n_tiles),
                                        out.ctypes.data_as(C.POINTER(C.c_ubyte))))
    return out


def host_zone_curve_chunk(n_zones, rows, scratch_bytes=32 << 20):
    """PvAmdHostZoneCurveChunk: the steps of an accumulate pass one pair of in-run curve launches takes"""
    n = lib().PvAmdHostZoneCurveChunk(int(n_zones), int(rows), int(scratch_bytes))
    if n < 0:
        raise PlaneverbError(last_error())
    return n


# PVA_ZONE_DECAY_*: how the cells' samples are put into the time slots of a zone's ensemble decay curve
PVA_ZONE_DECAY_ABSOLUTE, PVA_ZONE_DECAY_ONSET = 0, 1
ZONE_DECAY_ALIGN_NAMES = ("absolute", "onset")
# PvAmdZoneDecay (64 bytes)
ZONE_DECAY_DTYPE = np.dtype([("edt", "<f8"), ("t20", "<f8"), ("t30", "<f8"), ("e0", "<f8"), ("depth", "<f8"), ("n_edt", "<i4"),
                             ("n_t20", "<i4"), ("n_t30", "<i4"), ("n_cells", "<i4"), ("t_first", "<i4"), ("t_last", "<i4")])
assert ZONE_DECAY_DTYPE.itemsize == 64
_dp = C.POINTER(C.c_double)


def _zone_decay_align(align):
    if isinstance(align, str):
        if align not in ZONE_DECAY_ALIGN_NAMES:
            raise ValueError("zone decay: align is one of %s" % ", ".join(ZONE_DECAY_ALIGN_NAMES))
        return ZONE_DECAY_ALIGN_NAMES.index(align)
    return int(align)


def host_zone_decay(p, delay, fs, labels, n_zones=None, align="absolute"):
    """PvAmdHostZoneDecay: the zone decay of include/planeverb_amd.h (PvAmdZoneDecay) on the CPU -- p = float32 [T, gx, gy]
    (plane t as Solver.history_plane(t)[:gx, :gy]), delay = float32 [gx, gy] (the onset map, FLT_MAX: none), labels = uint8
    [gx, gy] (0: no zone, 1 .. n_zones; None: the largest label), align "absolute" or "onset"; (records [n_zones] of
    ZONE_DECAY_DTYPE, etc float64 [n_zones, T], edc float64 [n_zones, T])"""
    h = np.ascontiguousarray(p, np.float32)
    d = np.ascontiguousarray(delay, np.float32)
    lab, n = _zone_labels(labels, n_zones)
    if h.ndim != 3 or d.shape != h.shape[1:] or lab.shape != h.shape[1:]:
        raise ValueError("host_zone_decay: a history [T, gx, gy], onsets [gx, gy] and labels [gx, gy]")
    T = h.shape[0]
    out = np.zeros(max(n, 0), ZONE_DECAY_DTYPE)
    etc, edc = np.zeros((max(n, 0), T)), np.zeros((max(n, 0), T))
    _check(lib().PvAmdHostZoneDecay(_f(h) if h.size else None, _f(d) if d.size else None, h.shape[1], h.shape[2], T, int(fs),
                                    lab.ctypes.data_as(C.POINTER(C.c_ubyte)), n, _zone_decay_align(align), out.ctypes.data_as(_vp),
                                    etc.ctypes.data_as(_dp), edc.ctypes.data_as(_dp)))
    return out, etc, edc


# PvAmdZoneBandDecay (96 bytes): PvAmdZoneDecay with the clarity of the curve behind depth
ZONE_BAND_DECAY_DTYPE = np.dtype([("edt", "<f8"), ("t20", "<f8"), ("t30", "<f8"), ("e0", "<f8"), ("depth", "<f8"), ("c50", "<f8"),
                                  ("c80", "<f8"), ("d50", "<f8"), ("ts", "<f8"), ("n_edt", "<i4"), ("n_t20", "<i4"), ("n_t30", "<i4"),
                                  ("n_cells", "<i4"), ("t_first", "<i4"), ("t_last", "<i4")])
assert ZONE_BAND_DECAY_DTYPE.itemsize == 96


def host_zone_band_decay(p, delay, fs, labels, coefs, n_zones=None, align="absolute"):
    """PvAmdHostZoneBandDecay: the zone band decay of include/planeverb_amd.h (PvAmdZoneBandDecay) on the CPU -- p, delay, labels,
    n_zones and align as for host_zone_decay, coefs = float32 [n_bands, 10] (host_band_coefs / Solver.band_coefs); (records
    [n_zones, n_bands] of ZONE_BAND_DECAY_DTYPE, etc float64 [n_zones, n_bands, T], edc float64 [n_zones, n_bands, T])"""
    h = np.ascontiguousarray(p, np.float32)
    d = np.ascontiguousarray(delay, np.float32)
    c = np.ascontiguousarray(coefs, np.float32).reshape(-1, 10)
    lab, n = _zone_labels(labels, n_zones)
    if h.ndim != 3 or d.shape != h.shape[1:] or lab.shape != h.shape[1:]:
        raise ValueError("host_zone_band_decay: a history [T, gx, gy], onsets [gx, gy] and labels [gx, gy]")
    T, nb = h.shape[0], c.shape[0]
    out = np.zeros((max(n, 0), nb), ZONE_BAND_DECAY_DTYPE)
    etc, edc = np.zeros((max(n, 0), nb, T)), np.zeros((max(n, 0), nb, T))
    _check(lib().PvAmdHostZoneBandDecay(_f(h) if h.size else None, _f(d) if d.size else None, h.shape[1], h.shape[2], T, int(fs),
                                        lab.ctypes.data_as(C.POINTER(C.c_ubyte)), n, _f(c) if c.size else None, nb,
                                        _zone_decay_align(align), out.ctypes.data_as(_vp), etc.ctypes.data_as(_dp),
                                        edc.ctypes.data_as(_dp)))
    return out, etc, edc


def host_zone_curve_clarity(etc, fs, j0):
    """PvAmdHostZoneCurveClarity: float64 [4] = c50, c80, d50, ts of the energy-time curve etc[T] whose beginning is slot j0 -- the
    clarity rule of include/planeverb_amd.h (PvAmdZoneBandDecay); with the etc of Solver.zone_decay: the broadband curve's"""
    e = np.ascontiguousarray(etc, np.float64).reshape(-1)
    out = np.zeros(4)
    _check(lib().PvAmdHostZoneCurveClarity(e.ctypes.data_as(_dp) if e.size else None, int(e.size), int(fs), int(j0),
                                           out.ctypes.data_as(_dp)))
    return out


def host_cells(size_x, size_y, res, x, z):
    v = [C.c_int() for _ in range(5)]
    _check(lib().PvAmdHostCells(float(size_x), float(size_y), int(res), float(x), float(z), *v))
    return (v[0].value, v[1].value), ((v[2].value, v[3].value) if v[4].value else None)


def clock_probe(device=0):
    """(MHz by a timed s_sleep, MHz by s_memtime) of the device's shader clock at this moment (PvAmdClockProbe)"""
    m = C.c_float(0.0)
    v = lib().PvAmdClockProbe(int(device), C.byref(m))
    return float(v), float(m.value)


def bandwidth_probe(device=0):
    """the device's own streaming bandwidth in GB/s (PvAmdBandwidthProbe): copy with 16 B and with 4 B per lane (bytes read +
    written per second), read only, write only"""
    v = (C.c_float * 4)()
    _check(lib().PvAmdBandwidthProbe(int(device), v))
    return {"copy_x4": float(v[0]), "copy_dword": float(v[1]), "read_dword": float(v[2]), "write_dword": float(v[3])}


# PVA_LIBM_*: the forms of csrc/pv_libm.h that libm_probe evaluates
LIBM_FORMS = ("log10", "log10_nonneg", "log10_nonneg_tab", "log10_normal_tab", "log10_normal_batch", "pow_08", "pow_23",
              "pow_nonneg_08", "pow_nonneg_23", "pow_nonneg_tab_08", "pow_nonneg_tab_23")
LIBM_NORMAL_ONLY = ("log10_normal_tab", "log10_normal_batch")  # defined for positive normal finite inputs only


def libm_probe(form, x, on_device=True):
    """PvAmdLibmProbe: float32, the shape of x -- the library's own log10f / powf in the form named (LIBM_FORMS, or its index) of
    every x, evaluated by the device compile on the current device (the tables in LDS) or by the same source on the host"""
    f = LIBM_FORMS.index(form) if isinstance(form, str) else int(form)
    a = np.ascontiguousarray(x, np.float32)
    out = np.empty_like(a)
    _check(lib().PvAmdLibmProbe(f, _f(a) if a.size else None, _f(out) if a.size else None, int(a.size), 1 if on_device else 0))
    return out


def device_count():
    return lib().PvAmdDeviceCount()


# --------------------------------------------------------------------------------------------------------------
# batch solver
# --------------------------------------------------------------------------------------------------------------

def batch_solver_options(n):
    """Solver options for grids of about n x n cells that are run in batches (run_batch): the mirror-pair tiles whose
    batched kernel has the edge-tile arm (grid-border tiles on the air path, tile class 2), measured on MI355X:
    +13 % at 512^2, +25 % at 1024^2 over the default tile of the size"""
    if n <= 768:
        return dict(steps_per_launch=8, tile_rows=40, edge_tiles=1, aux_streams=1)
    if n <= 1536:
        return dict(steps_per_launch=10, tile_rows=36, edge_tiles=1, aux_streams=1)
    return dict(steps_per_launch=12, tile_rows=36, edge_tiles=1, aux_streams=1)


def shard_plan(n_runs, world, rank, n_local_solvers):
    """PvAmdShardPlan: [(run index, local solver index), ...] of this rank (run k -> rank k mod world)"""
    cap = max(1, (n_runs + max(world, 1) - 1) // max(world, 1))
    r, s = (C.c_int * cap)(), (C.c_int * cap)()
    n = lib().PvAmdShardPlan(int(n_runs), int(world), int(rank), int(n_local_solvers), r, s, cap)
    return [(r[i], s[i]) for i in range(min(n, cap))]


class Comm:
    """RCCL communicator of the sharded runs (PvAmdComm*): one per process, bound to the process's HIP device"""

    @staticmethod
    def unique_id():
        buf = C.create_string_buffer(128)
        _check(lib().PvAmdCommUniqueId(buf))
        return buf.raw

    def __init__(self, unique_id, rank, world, device):
        assert len(unique_id) == 128
        self._h = lib().PvAmdCommCreate(unique_id, int(rank), int(world), int(device))
        if not self._h:
            raise PlaneverbError(last_error())
        self.rank, self.world = rank, world

    def all_gather(self, mine):
        mine = np.ascontiguousarray(mine, np.float32).ravel()
        out = np.empty(self.world * mine.size, np.float32)
        _check(lib().PvAmdCommAllGather(self._h, _f(mine), mine.size, _f(out)))
        return out.reshape(self.world, -1)

    def close(self):
        if getattr(self, "_h", None):
            lib().PvAmdCommDestroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def plan_segments(air, tile_rows, max_tile_columns, target):
    """PvAmdPlanSegments: the row-streaming segments (PVA_OPT_STREAM_ROWS) covering the air tiles of a [ntx, nty] 0/1
    array: int array [n, 4] of (first array row, rows, first tile column, tile columns)"""
    a = np.ascontiguousarray(air, np.uint8)
    ntx, nty = a.shape
    cap = 2 * a.size + 8
    out = np.zeros((cap, 4), np.int32)
    n = lib().PvAmdPlanSegments(a.ctypes.data_as(C.POINTER(C.c_ubyte)), ntx, nty, int(tile_rows), int(max_tile_columns),
                                int(target), out.ctypes.data_as(C.POINTER(C.c_int)), cap)
    return out[:min(n, cap)].copy()


def run_sharded(solvers, listeners, emitters, rank=0, world=1, comm=None):
    """PvAmdRunSharded: listeners [n, 3], emitters [n, E, 3] -> float32 [n, E, 8] on every rank"""
    L = np.ascontiguousarray(listeners, np.float32).reshape(-1, 3)
    Em = np.ascontiguousarray(emitters, np.float32).reshape(len(L), -1, 3)
    n, E = len(L), Em.shape[1]
    hs = (_vp * len(solvers))(*[sv._h for sv in solvers])
    out = (PlaneverbOutput * max(1, n * E))()
    _check(lib().PvAmdRunSharded(hs, len(solvers), _f(L), n, _f(Em), E, int(rank), int(world),
                                 comm._h if comm is not None else None, out))
    return np.frombuffer(out, np.float32).reshape(-1, 8)[:n * E].reshape(n, E, 8).copy()


class Bake:
    """A baked listener-probe table (PvAmdBake*, include/planeverb_amd.h Part 4): probes (x0 + i sx, 0, z0 + j sz), k = j nx + i;
    per probe the block of emitter-lattice nodes (stride `stride` in result cells) its run reached, queried by interpolation.

        b = Bake(solver, stride, x0, z0, sx, sz, nx, nz); b.run([s0, s1]); b.save(path); Bake.load(path).query(L, E)
    """

    def __init__(self, like, stride, x0, z0, sx, sz, nx, nz):
        self._h = lib().PvAmdBakeCreate(like._h, int(stride), float(x0), float(z0), float(sx), float(sz), int(nx), int(nz))
        if not self._h:
            raise PlaneverbError(last_error())

    @classmethod
    def load(cls, path):
        h = lib().PvAmdBakeLoad(os.fsencode(path))
        if not h:
            raise PlaneverbError(last_error())
        b = cls.__new__(cls)
        b._h = h
        return b

    def close(self):
        if getattr(self, "_h", None):
            lib().PvAmdBakeDestroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def run(self, solvers, rank=0, world=1):
        """bake the probes k % world == rank on these solvers (round-robin, one run in flight each)"""
        hs = (_vp * len(solvers))(*[sv._h for sv in solvers])
        _check(lib().PvAmdBakeRun(self._h, hs, len(solvers), int(rank), int(world)))

    def merge(self, other):
        _check(lib().PvAmdBakeMerge(self._h, other._h))

    def save(self, path):
        _check(lib().PvAmdBakeSave(self._h, os.fsencode(path)))

    def info(self):
        i = PvAmdBakeInfo()
        _check(lib().PvAmdBakeGetInfo(self._h, i))
        return {f: getattr(i, f) for f, _ in PvAmdBakeInfo._fields_}

    def probe(self, k):
        """(state5 int32 [5] = state, i0, j0, ni, nj;  records float32 [ni, nj, 9])"""
        st = np.zeros(5, np.int32)
        n = lib().PvAmdBakeProbe(self._h, int(k), st.ctypes.data_as(C.POINTER(C.c_int)), None)
        if n < 0:
            raise PlaneverbError(last_error())
        rec = np.zeros(max(n, 1) * 9, np.float32)
        _check(0 if lib().PvAmdBakeProbe(self._h, int(k), st.ctypes.data_as(C.POINTER(C.c_int)), _f(rec)) == n else -1)
        return st, rec[:n * 9].reshape(int(st[3]), int(st[4]), 9)

    def _pairs(self, listeners, emitters):
        L = np.ascontiguousarray(listeners, np.float32).reshape(-1, 3)
        E = np.ascontiguousarray(emitters, np.float32).reshape(-1, 3)
        if len(L) != len(E):
            raise ValueError("listeners and emitters must pair up")
        return L, E, np.zeros((max(len(L), 1), 8), np.float32)

    def query(self, listeners, emitters):
        """listeners [n, 3], emitters [n, 3] -> float32 [n, 8] (CPU)"""
        L, E, out = self._pairs(listeners, emitters)
        _check(lib().PvAmdBakeQuery(self._h, _f(L), _f(E), len(L), _f(out)))
        return out[:len(L)]

    def query_device(self, listeners, emitters, device=0):
        """the same on a HIP device (bit-identical)"""
        L, E, out = self._pairs(listeners, emitters)
        _check(lib().PvAmdBakeQueryDevice(self._h, int(device), _f(L), _f(E), len(L), _f(out)))
        return out[:len(L)]


def compute_efree(size_x, size_y, res, device=0):
    """FreeGrid energy of a config (FreeGrid.cpp:71-110): computed once, handed to every slab rank"""
    e = C.c_float()
    _check(lib().PvAmdComputeEfree(float(size_x), float(size_y), int(res), int(device), e))
    return e.value


class SlabRank:
    """ONE slab of a decomposed grid, owned by this process (PvAmdCreateSlabRank + PvAmdSlab*): the per-rank primitives of
    planeverb_amd.dist_slabs.  Buffers that cross ranks are numpy arrays."""

    def __init__(self, size_x, size_y, res, device, index, count, efree, **options):
        self.solver = Solver.__new__(Solver)
        self.solver._h = lib().PvAmdCreateSlabRank(float(size_x), float(size_y), int(res), int(device), int(index), int(count))
        if not self.solver._h:
            raise PlaneverbError(last_error())
        self._h = self.solver._h
        keys = {"steps_per_launch": PVA_OPT_STEPS_PER_LAUNCH, "tile_rows": PVA_OPT_TILE_ROWS, "num_steps": PVA_OPT_NUM_STEPS}
        for k, v in options.items():
            _check(lib().PvAmdSetOption(self._h, keys[k], int(v)))
        _check(lib().PvAmdSlabSetEfree(self._h, float(efree)))
        self.index, self.count = index, count
        self.num_launches = lib().PvAmdSlabNumLaunches(self._h)
        self.halo_floats = lib().PvAmdSlabHaloFloats(self._h)
        self.history_floats = lib().PvAmdSlabHistoryFloats(self._h)

    def close(self):
        self.solver.close()
        self._h = None

    def add_geometry(self, aabb):
        return lib().PvAmdAddGeometry(self._h, *[float(v) for v in aabb])

    def begin(self, listener):
        _check(lib().PvAmdSlabBegin(self._h, *[float(v) for v in listener]))

    def launch(self, li):
        _check(lib().PvAmdSlabLaunch(self._h, int(li)))

    def export_halo(self, side):
        out = np.empty(self.halo_floats, np.float32)
        _check(lib().PvAmdSlabExportHalo(self._h, int(side), _f(out)))
        return out

    def import_halo(self, side, buf):
        buf = np.ascontiguousarray(buf, np.float32)
        assert buf.size == self.halo_floats
        _check(lib().PvAmdSlabImportHalo(self._h, int(side), _f(buf)))

    # the same four transfers with raw addresses of buffers that may live on the slab's device (torch tensors: .data_ptr()):
    # what an RCCL transport uses, nothing is staged through the host (dist_slabs.TorchTransport)
    def export_halo_to(self, side, ptr):
        _check(lib().PvAmdSlabExportHalo(self._h, int(side), C.cast(C.c_void_p(int(ptr)), _fp)))

    def import_halo_from(self, side, ptr):
        _check(lib().PvAmdSlabImportHalo(self._h, int(side), C.cast(C.c_void_p(int(ptr)), _fp)))

    def export_edge_history_to(self, ptr):
        _check(lib().PvAmdSlabExportEdgeHistory(self._h, C.cast(C.c_void_p(int(ptr)), _fp)))

    def import_above_history_from(self, ptr):
        _check(lib().PvAmdSlabImportAboveHistory(self._h, C.cast(C.c_void_p(int(ptr)), _fp)))

    def export_edge_history(self):
        out = np.empty(self.history_floats, np.float32)
        _check(lib().PvAmdSlabExportEdgeHistory(self._h, _f(out)))
        return out

    def import_above_history(self, buf):
        buf = np.ascontiguousarray(buf, np.float32)
        assert buf.size == self.history_floats
        _check(lib().PvAmdSlabImportAboveHistory(self._h, _f(buf)))

    def analyze(self):
        _check(lib().PvAmdSlabAnalyze(self._h))

    def window_block(self):
        """(info4 int32 [row0 of the whole grid, col0, rows, cols], float32 [7, rows, cols])"""
        info = (C.c_int * 4)()
        n = lib().PvAmdSlabWindowBlock(self._h, info, None, 0)
        if n < 0:
            raise PlaneverbError(last_error())
        data = np.empty(max(n, 0), np.float32)
        if n > 0 and lib().PvAmdSlabWindowBlock(self._h, info, _f(data), n) != n:
            raise PlaneverbError(last_error())
        return np.array(list(info), np.int32), data


class SlabRoot:
    """whole-grid result maps of a decomposed grid (rank 0): far cells, the ranks' blocks, the direction descent"""

    def __init__(self, slab_rank, device=0):
        self._h = lib().PvAmdSlabRootCreate(slab_rank._h, int(device))
        if not self._h:
            raise PlaneverbError(last_error())
        i = PvAmdInfo()
        _check(lib().PvAmdGetInfo(slab_rank._h, i))
        self.gx, self.gy = i.gx, i.gy

    def close(self):
        if getattr(self, "_h", None):
            lib().PvAmdSlabRootDestroy(self._h)
            self._h = None

    def begin(self, listener):
        _check(lib().PvAmdSlabRootBegin(self._h, *[float(v) for v in listener]))

    def import_block(self, info4, data):
        info = (C.c_int * 4)(*[int(v) for v in info4])
        data = np.ascontiguousarray(data, np.float32)
        _check(lib().PvAmdSlabRootImportBlock(self._h, info, _f(data) if data.size else None))

    def finish(self):
        _check(lib().PvAmdSlabRootFinish(self._h))

    def get_output(self, emitter):
        o = PlaneverbOutput()
        _check(lib().PvAmdSlabRootGetOutput(self._h, *[float(v) for v in emitter], o))
        return o

    def results(self):
        res = np.empty((self.gx, self.gy, 8), np.float32)
        delay = np.empty((self.gx, self.gy), np.float32)
        _check(lib().PvAmdSlabRootCopyResults(self._h, _f(res), _f(delay)))
        return res, delay


def run_batch(solvers, listeners, wait=True):
    """PvAmdRunBatch: len(solvers) <= 8 independent runs (one listener each) advanced by ONE launch per K steps.
    The solvers must share device, grid and tile configuration; afterwards each holds its own run's results."""
    n = len(solvers)
    if n != len(listeners):
        raise ValueError("one listener position per solver")
    hs = (_vp * n)(*[sv._h for sv in solvers])
    xyz = (C.c_float * (3 * n))(*[float(v) for L in listeners for v in L])
    _check(lib().PvAmdRunBatch(hs, n, xyz, 1 if wait else 0))


class Solver:
    """Grid + FreeGrid + Analyzer of one config on one MI355X (PvAmd* handle API)."""

    def __init__(self, size_x, size_y, res, device=0, slabs=None, **options):
        """slabs = list of HIP devices, one per row slab: ONE grid decomposed into len(slabs) slabs (PvAmdCreateSlabs;
        all devices equal = several slabs on one GPU).  Same results, bit for bit."""
        if slabs is not None:
            dev = (C.c_int * len(slabs))(*[int(d) for d in slabs])
            self._h = lib().PvAmdCreateSlabs(float(size_x), float(size_y), int(res), dev, len(slabs))
        else:
            self._h = lib().PvAmdCreate(float(size_x), float(size_y), int(res), int(device))
        if not self._h:
            raise PlaneverbError(last_error())
        keys = {"dense_history": PVA_OPT_DENSE_HISTORY, "num_steps": PVA_OPT_NUM_STEPS,
                "skip_analysis": PVA_OPT_SKIP_ANALYSIS, "use_graph": PVA_OPT_USE_GRAPH,
                "steps_per_launch": PVA_OPT_STEPS_PER_LAUNCH, "tile_rows": PVA_OPT_TILE_ROWS,
                "no_free_grid": PVA_OPT_NO_FREE_GRID, "time_kernels": PVA_OPT_TIME_KERNELS,
                "tile_order": PVA_OPT_TILE_ORDER, "small_grid_kernel": PVA_OPT_SMALL_GRID_KERNEL,
                "packed_math": PVA_OPT_PACKED_MATH, "streaming_analysis": PVA_OPT_STREAMING_ANALYSIS,
                "stream_rows": PVA_OPT_STREAM_ROWS, "merged_launch": PVA_OPT_MERGED_LAUNCH,
                "edge_tiles": PVA_OPT_EDGE_TILES, "row_bands": PVA_OPT_ROW_BANDS,
                "patch_kernel": PVA_OPT_PATCH_KERNEL, "patch_strip": PVA_OPT_PATCH_STRIP,
                "lazy_far_cells": PVA_OPT_LAZY_FAR_CELLS, "stream_fuse": PVA_OPT_STREAM_FUSE, "aux_streams": PVA_OPT_AUX_STREAMS,
                "resident_kernel": PVA_OPT_RESIDENT_KERNEL, "rt60_lanes": PVA_OPT_RT60_LANES,
                "debug_lose_first_capture": PVA_OPT_DEBUG_LOSE_FIRST_CAPTURE, "stream_priority": PVA_OPT_STREAM_PRIORITY,
                "alternate_sweeps": PVA_OPT_ALTERNATE_SWEEPS, "xcd_regions": PVA_OPT_XCD_REGIONS,
                "analysis_fork": PVA_OPT_ANALYSIS_FORK, "fused_analysis": PVA_OPT_FUSED_ANALYSIS,
                "reach_bound": PVA_OPT_REACH_BOUND, "resident_window": PVA_OPT_RESIDENT_WINDOW}
        for k, v in options.items():
            _check(lib().PvAmdSetOption(self._h, keys[k], int(v)))
        self.info = PvAmdInfo()
        _check(lib().PvAmdGetInfo(self._h, self.info))
        i = self.info
        self.gx, self.gy, self.T, self.fs, self.dx, self.dt, self.efree = i.gx, i.gy, i.T, i.fs, i.dx, i.dt, i.efree
        self._pulse_len = host_grid_info(size_x, size_y, res).T  # (the grid's own pulse table: T may differ, num_steps)

    def close(self):
        if getattr(self, "_h", None):
            lib().PvAmdDestroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def slab_info(self):
        i = PvAmdSlabInfo()
        _check(lib().PvAmdGetSlabInfo(self._h, i))
        return i

    def load_scene(self, path):
        n = lib().PvAmdLoadScene(self._h, path.encode())
        if n < 0:
            raise PlaneverbError(last_error())
        return n

    def save_scene(self, path):
        _check(lib().PvAmdSaveScene(self._h, path.encode()))

    def add_geometry(self, aabb):
        return lib().PvAmdAddGeometry(self._h, *[float(v) for v in aabb])

    def update_geometry(self, gid, aabb):
        _check(lib().PvAmdUpdateGeometry(self._h, int(gid), *[float(v) for v in aabb]))

    def remove_geometry(self, gid):
        _check(lib().PvAmdRemoveGeometry(self._h, int(gid)))

    def add_shape(self, vertices, absorption):
        """a convex polygon of 3..8 vertices (grid metres); returns its shape id (PlaneverbError if refused)"""
        a, n = _xy(vertices)
        sid = lib().PvAmdAddShape(self._h, _f(a), n, float(absorption))
        if sid < 0:
            raise PlaneverbError(last_error())
        return sid

    def add_oriented_box(self, px, py, w, h, ax, ay, absorption):
        """an oriented box: centre, full width along the axis (ax, ay), full height; returns its shape id"""
        sid = lib().PvAmdAddOrientedBox(self._h, float(px), float(py), float(w), float(h), float(ax), float(ay), float(absorption))
        if sid < 0:
            raise PlaneverbError(last_error())
        return sid

    def update_shape(self, sid, vertices, absorption):
        a, n = _xy(vertices)
        _check(lib().PvAmdUpdateShape(self._h, int(sid), _f(a), n, float(absorption)))

    def update_oriented_box(self, sid, px, py, w, h, ax, ay, absorption):
        _check(lib().PvAmdUpdateOrientedBox(self._h, int(sid), float(px), float(py), float(w), float(h), float(ax), float(ay),
                                            float(absorption)))

    def _added(self, sid):
        if sid < 0:
            raise PlaneverbError(last_error())
        return sid

    def add_disc(self, cx, cy, radius, absorption):
        """a disc (grid metres); returns its shape id (PlaneverbError if refused)"""
        return self._added(lib().PvAmdAddDisc(self._h, float(cx), float(cy), float(radius), float(absorption)))

    def update_disc(self, sid, cx, cy, radius, absorption):
        _check(lib().PvAmdUpdateDisc(self._h, int(sid), float(cx), float(cy), float(radius), float(absorption)))

    def add_capsule(self, a, b, radius, absorption):
        """a thick wall segment a -> b of half thickness radius; returns its shape id"""
        return self._added(lib().PvAmdAddCapsule(self._h, float(a[0]), float(a[1]), float(b[0]), float(b[1]), float(radius),
                                                 float(absorption)))

    def update_capsule(self, sid, a, b, radius, absorption):
        _check(lib().PvAmdUpdateCapsule(self._h, int(sid), float(a[0]), float(a[1]), float(b[0]), float(b[1]), float(radius),
                                        float(absorption)))

    def add_wall_path(self, points, radius, absorption):
        """a polyline of 2..64 points, one capsule per segment, as ONE shape; returns its shape id"""
        p, n = _xy(points)
        return self._added(lib().PvAmdAddWallPath(self._h, _f(p), n, float(radius), float(absorption)))

    def update_wall_path(self, sid, points, radius, absorption):
        p, n = _xy(points)
        _check(lib().PvAmdUpdateWallPath(self._h, int(sid), _f(p), n, float(radius), float(absorption)))

    def add_polygon(self, vertices, absorption):
        """a simple polygon of 3..64 vertices, concave allowed, either winding; returns its shape id"""
        p, n = _xy(vertices)
        return self._added(lib().PvAmdAddPolygon(self._h, _f(p), n, float(absorption)))

    def update_polygon(self, sid, vertices, absorption):
        p, n = _xy(vertices)
        _check(lib().PvAmdUpdatePolygon(self._h, int(sid), _f(p), n, float(absorption)))

    def remove_shape(self, sid):
        _check(lib().PvAmdRemoveShape(self._h, int(sid)))

    def add_mesh(self, vertices, triangles, absorption, mode=MESH_SOLID, radius=0.0):
        """a triangle mesh (nv x 3 world (x, y, z), y = height; nt x 3 indices), kept on the device and sliced at the solver's
        slice height: MESH_SOLID fills the section (even-odd, holes included), MESH_SHELL covers within radius of it.  Returns
        the mesh id (a table of its own; PlaneverbError if refused)"""
        v, t, tp = _mesh(vertices, triangles)
        return self._added(lib().PvAmdAddMesh(self._h, _f(v), v.shape[0], tp, t.shape[0], float(absorption), int(mode),
                                              float(radius)))

    def update_mesh(self, mid, vertices, triangles, absorption, mode=MESH_SOLID, radius=0.0):
        v, t, tp = _mesh(vertices, triangles)
        _check(lib().PvAmdUpdateMesh(self._h, int(mid), _f(v), v.shape[0], tp, t.shape[0], float(absorption), int(mode),
                                     float(radius)))

    def set_mesh_transform(self, mid, transform):
        """3 x 4 row-major affine transform of the mesh's vertices; counts as an update (the mesh becomes the most recent)"""
        m, mp = _m12(np.eye(3, 4) if transform is None else transform)
        _check(lib().PvAmdSetMeshTransform(self._h, int(mid), mp))

    def remove_mesh(self, mid):
        _check(lib().PvAmdRemoveMesh(self._h, int(mid)))

    def set_slice_height(self, h):
        """the world height at which every mesh is sliced (0 by default); a change re-slices them at the next run"""
        _check(lib().PvAmdSetSliceHeight(self._h, float(h)))

    @property
    def slice_height(self):
        return float(lib().PvAmdGetSliceHeight(self._h))

    def mesh_section(self, mid):
        """the mesh's section as the device sliced it: (segments nt x 4 float32 (a.x, a.z, b.x, b.z), valid nt uint8)"""
        nt = lib().PvAmdMeshTriangles(self._h, int(mid))
        if nt < 0:
            raise PlaneverbError("invalid mesh id")
        seg = np.empty((nt, 4), np.float32)
        valid = np.empty(nt, np.uint8)
        _check(lib().PvAmdCopyMeshSection(self._h, int(mid), _f(seg), valid.ctypes.data_as(C.POINTER(C.c_ubyte))))
        return seg, valid

    def set_grid_boundary(self, r4):
        """absorption R of the grid edges x = 0, x = gx, y = 0 (world z = 0), y = gy, as add_geometry takes it: 0 = absorbing
        (the default), 1 = rigid.  Takes effect at the next run."""
        a = np.ascontiguousarray(r4, np.float32).reshape(-1)
        if a.size != 4:
            raise ValueError("four absorption values: x = 0, x = gx, y = 0, y = gy")
        _check(lib().PvAmdSetGridBoundary(self._h, _f(a)))

    def grid_boundary(self):
        out = np.zeros(4, np.float32)
        _check(lib().PvAmdGetGridBoundary(self._h, _f(out)))
        return out

    def set_edge_layer(self, w4):
        """widths in cells (0..64, 0 = none) of graded absorbing layers along the grid edges x = 0, x = gx, y = 0, y = gy
        (include/planeverb_amd.h PvAmdSetEdgeLayer).  Cells inside a layer get results, but not physical ones.  Takes effect
        at the next run."""
        a = _w4(w4)
        _check(lib().PvAmdSetEdgeLayer(self._h, a.ctypes.data_as(C.POINTER(C.c_int))))
        _check(lib().PvAmdGetInfo(self._h, self.info))  # (residentKernel: 0 while a layer is set)

    def edge_layer(self):
        out = np.zeros(4, np.int32)
        _check(lib().PvAmdGetEdgeLayer(self._h, out.ctypes.data_as(C.POINTER(C.c_int))))
        return out

    def set_edge_layer_split(self, w4, r0=EDGE_LAYER_SPLIT_R0):
        """set_edge_layer with the split-field model (include/planeverb_amd.h PvAmdSetEdgeLayerSplit): each layer cell's
        pressure is carried as an x and a y part, each damped by its own axis; r0 = the tables' design reflection, 0 < r0 < 1.
        set_edge_layer afterwards selects the unsplit model again.  Takes effect at the next run."""
        a = _w4(w4)
        _check(lib().PvAmdSetEdgeLayerSplit(self._h, a.ctypes.data_as(C.POINTER(C.c_int)), float(r0)))
        _check(lib().PvAmdGetInfo(self._h, self.info))  # (residentKernel: 0 while a layer is set)

    def edge_layer_model(self):
        """("split", r0) or ("unsplit", 0.1): the model of the solver's edge layers"""
        sp, r0 = C.c_int(0), C.c_double(0.0)
        _check(lib().PvAmdGetEdgeLayerModel(self._h, C.byref(sp), C.byref(r0)))
        return ("split" if sp.value else "unsplit"), r0.value

    def run(self, listener):
        _check(lib().PvAmdRun(self._h, *[float(v) for v in listener]))

    def run_async(self, listener):
        _check(lib().PvAmdRunAsync(self._h, *[float(v) for v in listener]))

    def run_async_after(self, prev, listener):
        """a run that continues `prev`'s result map (PvAmdRunAsyncAfter: two solvers taking turns on one sequence of iterations)"""
        _check(lib().PvAmdRunAsyncAfter(self._h, prev._h, *[float(v) for v in listener]))

    def sync(self):
        _check(lib().PvAmdSync(self._h))

    def run_steps(self, nsteps, with_pulse=False, listener=(0.0, 0.0, 0.0)):
        _check(lib().PvAmdRunSteps(self._h, int(nsteps), int(with_pulse), float(listener[0]), float(listener[2])))

    def last_run_resident_window(self):
        """True when the last run went out as one resident-kernel launch over the window around the listener's room"""
        rc = lib().PvAmdLastRunResidentWindow(self._h)
        if rc < 0:
            raise PlaneverbError(last_error())
        return rc == 1

    def last_run_one_xcd(self):
        """True when the last run's resident-kernel launch handed its tiles over through one XCD's L2"""
        rc = lib().PvAmdLastRunOneXcd(self._h)
        if rc < 0:
            raise PlaneverbError(last_error())
        return rc == 1

    def timings(self):
        t = PvAmdTimings()
        _check(lib().PvAmdGetTimings(self._h, t))
        return t

    def set_emitters(self, emitters):
        """streaming-analysis mode: the emitter positions whose wet gain / RT60 are computed"""
        e = np.ascontiguousarray(emitters, np.float32).reshape(-1, 3)
        _check(lib().PvAmdSetEmitters(self._h, _f(e), len(e)))

    def get_output(self, emitter):
        o = PlaneverbOutput()
        _check(lib().PvAmdGetOutput(self._h, *[float(v) for v in emitter], o))
        return o

    def set_output_queries(self, emitters):
        """emitter positions whose outputs every following run leaves in pinned host memory (<= 64)"""
        e = np.ascontiguousarray(np.asarray(emitters, np.float32).reshape(-1, 3))
        self._nq = len(e)
        _check(lib().PvAmdSetOutputQueries(self._h, _f(e), len(e)))

    def queried_outputs(self):
        """float32 [n_queries, 8] of the last run (after sync; no GPU work)"""
        n = getattr(self, "_nq", 0)
        out = (PlaneverbOutput * max(n, 1))()
        _check(lib().PvAmdGetQueriedOutputs(self._h, out, n))
        return np.frombuffer(out, np.float32).reshape(-1, 8)[:n].copy()

    def set_query_records(self, kinds):
        """the per-cell record kinds (a mask of QREC_*) every following run computes for the cells of the output queries, in one
        launch inside the run and straight into pinned host memory; 0 (the default) selects none and frees the block"""
        _check(lib().PvAmdSetQueryRecords(self._h, int(kinds)))

    def _record_floats(self, floats, kind):
        n = floats(self._h, int(kind))
        if n < 0:
            raise PlaneverbError(last_error())
        return n

    def _read_records(self, read, kind, shape):
        """float32 [n_queries] + shape of ONE kind of either family, for the table the records follow"""
        n = getattr(self, "_nrq", 0) or getattr(self, "_nq", 0)
        out = np.empty((n,) + shape, np.float32)
        _check(read(self._h, int(kind), _f(out) if n else None, n))
        return out

    def query_record_kinds(self):
        return int(lib().PvAmdGetQueryRecordKinds(self._h))

    def query_record_floats(self, kind):
        """floats per query of ONE kind under the current settings (10, 8, 11, 1 + 3 nSlots, 10, 1 + 5 nW)"""
        return self._record_floats(lib().PvAmdQueryRecordFloats, kind)

    def queried_records(self, kind):
        """float32 [n_queries, floats] of ONE kind for the last run (waits for it; no GPU work): each row bit for bit what
        <kind>_at(position) returns after compute_<kind>() on the same run; NaN rows off the map and where no sound arrived"""
        return self._read_records(lib().PvAmdGetQueriedRecords, kind, (self.query_record_floats(kind),))

    def set_record_queries(self, positions):
        """positions of their own (<= RECORD_QUERIES_MAX) for the in-run records: while there are any, every following run
        computes the selected kinds for these cells instead of the output queries', and queried_records follows them;
        queried_outputs keeps serving the output queries.  An empty list returns to the output queries"""
        e = np.ascontiguousarray(np.asarray(positions, np.float32).reshape(-1, 3))
        _check(lib().PvAmdSetRecordQueries(self._h, _f(e) if len(e) else None, len(e)))
        self._nrq = len(e)

    def set_query_spectral_records(self, kinds):
        """the frequency-resolved record kinds (a mask of QSPEC_*: band metrics, modulation, spectrum) every following run
        computes for the cells the query records follow, in one launch of their own inside the run and straight into pinned
        host memory; 0 (the default) selects none and frees the block.  Independent of set_query_records"""
        _check(lib().PvAmdSetQuerySpectralRecords(self._h, int(kinds)))

    def query_spectral_kinds(self):
        return int(lib().PvAmdGetQuerySpectralKinds(self._h))

    def query_spectral_floats(self, kind):
        """floats per query of ONE kind under the current bands / bins (12 n, 15 n, 3 bins)"""
        return self._record_floats(lib().PvAmdQuerySpectralFloats, kind)

    def queried_spectral_records(self, kind):
        """float32 [n_queries, n, 12], [n_queries, n, 15] or [n_queries, bins, 3] of ONE kind for the last run (waits for it; no
        GPU work): each row bit for bit what band_metrics_at / modulation_at / spectrum_at(position) return after the whole-map
        pass on the same run; NaN rows off the map and where no sound arrived"""
        per = {QSPEC_BAND_METRICS: 12, QSPEC_MODULATION: 15, QSPEC_SPECTRUM: 3}.get(int(kind), 1)
        return self._read_records(lib().PvAmdGetQueriedSpectralRecords, kind, (self.query_spectral_floats(kind) // per, per))

    def set_emitter_records(self, time_kinds, spectral_kinds=0):
        """sparse-emitter mode: the record kinds (masks of QREC_* and of QSPEC_*) every following run computes for the registered
        emitters (set_emitters), inside the run and straight into pinned host memory; both 0 (the default) selects none"""
        _check(lib().PvAmdSetEmitterRecords(self._h, int(time_kinds), int(spectral_kinds)))

    def emitter_record_kinds(self):
        """(time kinds, spectral kinds)"""
        t, f = C.c_uint(0), C.c_uint(0)
        _check(lib().PvAmdGetEmitterRecordKinds(self._h, C.byref(t), C.byref(f)))
        return int(t.value), int(f.value)

    def emitter_cells(self):
        """int32 [n, 2]: the result cells (cx, cy) of the emitters set_emitters kept (it drops positions off the map), in the order
        of the emitter records"""
        n = lib().PvAmdGetEmitterCells(self._h, None, 0)
        if n < 0:
            raise PlaneverbError(last_error())
        out = np.zeros((n, 2), np.int32)
        if n and lib().PvAmdGetEmitterCells(self._h, out.ctypes.data_as(C.POINTER(C.c_int)), n) < 0:
            raise PlaneverbError(last_error())
        return out

    def emitter_records(self, kind, spectral=False):
        """float32 [n_emitters, floats] of ONE kind (QSPEC_* with spectral=True) for the last run (waits for it; no GPU work): row i
        bit for bit what <kind>_at returns at emitter_cells()[i] on a solver that keeps its history; NaN rows where no sound
        arrived.  The spectral kinds' rows are band after band (12 or 15 floats) or bin after bin (3 floats)"""
        fam = 1 if spectral else 0
        floats = lib().PvAmdEmitterRecordFloats(self._h, fam, int(kind))
        if floats < 0:
            raise PlaneverbError(last_error())
        n = len(self.emitter_cells())
        out = np.empty((n, floats), np.float32)
        _check(lib().PvAmdGetEmitterRecords(self._h, fam, int(kind), _f(out) if n else None, n))
        return out

    def emitter_trace(self, i):
        """float32 [T]: the pressure at kept emitter i at every step of the last sparse-emitter run"""
        out = np.empty(self.T, np.float32)
        _check(lib().PvAmdCopyEmitterTrace(self._h, int(i), _f(out)))
        return out

    def results(self):
        res = np.empty((self.gx, self.gy, 8), np.float32)
        delay = np.empty((self.gx, self.gy), np.float32)
        _check(lib().PvAmdCopyResults(self._h, _f(res), _f(delay)))
        return res, delay

    def results_block(self, r0, c0, nr, nc):
        """(records [nr, nc, 8], onsets [nr, nc]) of result cells [r0, r0 + nr) x [c0, c0 + nc)"""
        res = np.empty((nr, nc, 8), np.float32)
        delay = np.empty((nr, nc), np.float32)
        _check(lib().PvAmdCopyResultsBlock(self._h, int(r0), int(c0), int(nr), int(nc), _f(res), _f(delay)))
        return res, delay

    def impulse_response(self, cx, cy):
        out = np.empty((self.T, 3), np.float32)
        _check(lib().PvAmdGetImpulseResponse(self._h, int(cx), int(cy), _f(out)))
        return out

    def impulse_response_cells(self, cx, cy):
        """structured array [T] of reference Cells (pr, vx, vy, b, by)"""
        out = np.zeros(self.T, CELL_DTYPE)
        _check(lib().PvAmdGetImpulseResponseCells(self._h, int(cx), int(cy), out.ctypes.data_as(C.POINTER(PlaneverbCell))))
        return out

    def fields(self):
        shp = (self.gx + 1, self.gy + 1)
        pr, vx, vy = (np.empty(shp, np.float32) for _ in range(3))
        _check(lib().PvAmdCopyFields(self._h, _f(pr), _f(vx), _f(vy)))
        return pr, vx, vy

    def fields_local(self):
        """a slab rank's own rows of the final fields (PvAmdCopyFields on a slab copies the rows it owns)"""
        i = PvAmdInfo()
        _check(lib().PvAmdGetInfo(self._h, i))
        # rows owned = result rows, + the ghost row on the last slab: read generously, trim by what the library wrote
        bufs = [np.full((i.rows, i.gy + 1), np.nan, np.float32) for _ in range(3)]
        _check(lib().PvAmdCopyFields(self._h, _f(bufs[0]), _f(bufs[1]), _f(bufs[2])))
        n = int((~np.isnan(bufs[0][:, 0])).sum())
        return [b[:n] for b in bufs]

    def set_fields(self, pr, vx, vy):
        a = [np.ascontiguousarray(x, np.float32) for x in (pr, vx, vy)]
        _check(lib().PvAmdSetFields(self._h, _f(a[0]), _f(a[1]), _f(a[2])))

    def history_plane(self, t):
        out = np.empty((self.gx + 1, self.gy + 1), np.float32)
        _check(lib().PvAmdCopyHistoryPlane(self._h, int(t), _f(out)))
        return out

    def set_history_plane(self, t, plane):
        """PvAmdSetHistoryPlane, the inverse of history_plane (a test seam): plane = float32 [gx + 1, gy + 1] into the stored cells
        of step t of the last completed run; every analysis map becomes "not computed" """
        a = np.ascontiguousarray(plane, np.float32)
        if a.shape != (self.gx + 1, self.gy + 1):
            raise ValueError("set_history_plane: a plane [gx + 1, gy + 1], as history_plane returns it")
        _check(lib().PvAmdSetHistoryPlane(self._h, int(t), _f(a)))

    # The nine per-cell analysis kinds share four call shapes: compute -> device milliseconds, the whole map, a block of it, the
    # record at a position; `width` = the trailing dimensions of a record
    def _map_ms(self, fn):
        ms = C.c_float(0.0)
        _check(fn(self._h, C.byref(ms)))
        return ms.value

    def _map_all(self, fn, *width):
        out = np.empty((self.gx, self.gy) + width, np.float32)
        _check(fn(self._h, _f(out)))
        return out

    def _map_block(self, fn, r0, c0, nr, nc, *width):
        out = np.empty((nr, nc) + width, np.float32)
        _check(fn(self._h, int(r0), int(c0), int(nr), int(nc), _f(out)))
        return out

    def _map_at(self, fn, pos, *width, record=None):
        out = record() if record else np.empty(width, np.float32)
        _check(fn(self._h, *[float(v) for v in pos], out if record else _f(out)))
        return out.as_array() if record else out

    def compute_room_metrics(self):
        """room metrics (C50, C80, D50, Ts: ROOM_METRIC_NAMES) of the last completed run, one pass on the device; returns
        the pass's device time in milliseconds"""
        return self._map_ms(lib().PvAmdComputeRoomMetrics)

    def room_metrics(self):
        """float32 [gx, gy, 10] (ROOM_METRIC_NAMES); NaN where the cell has no onset in the run they were computed for"""
        return self._map_all(lib().PvAmdCopyRoomMetrics, 10)

    def room_metrics_block(self, r0, c0, nr, nc):
        """the records [nr, nc, 10] of result cells [r0, r0 + nr) x [c0, c0 + nc)"""
        return self._map_block(lib().PvAmdCopyRoomMetricsBlock, r0, c0, nr, nc, 10)

    def room_metrics_at(self, pos):
        """float32 [10] at an emitter position (the cell get_output reads); ten NaNs off the map"""
        return self._map_at(lib().PvAmdGetRoomMetrics, pos, record=PvAmdRoomMetrics)

    def compute_decay_times(self):
        """decay times (EDT, T20, T30: DECAY_TIME_NAMES) of the last completed run, two backward walks of its history on the
        device; returns the pass's device time in milliseconds"""
        return self._map_ms(lib().PvAmdComputeDecayTimes)

    def decay_times(self):
        """float32 [gx, gy, 8] (DECAY_TIME_NAMES); NaN where the cell has no onset in the run they were computed for, and in
        edt / t20 / t30 where the recorded curve does not fall through the range"""
        return self._map_all(lib().PvAmdCopyDecayTimes, 8)

    def decay_times_block(self, r0, c0, nr, nc):
        """the records [nr, nc, 8] of result cells [r0, r0 + nr) x [c0, c0 + nc)"""
        return self._map_block(lib().PvAmdCopyDecayTimesBlock, r0, c0, nr, nc, 8)

    def decay_times_at(self, pos):
        """float32 [8] at an emitter position (the cell get_output reads); eight NaNs off the map"""
        return self._map_at(lib().PvAmdGetDecayTimes, pos, record=PvAmdDecayTimes)

    def compute_echo_criterion(self):
        """echo criterion (Dietsch and Kraak, speech and music: ECHO_CRITERION_NAMES) of the last completed run, one forward
        pass over its history on the device; returns the pass's device time in milliseconds"""
        return self._map_ms(lib().PvAmdComputeEchoCriterion)

    def echo_criterion(self):
        """float32 [gx, gy, 10] (ECHO_CRITERION_NAMES); NaN where the cell has no onset in the run they were computed for"""
        return self._map_all(lib().PvAmdCopyEchoCriterion, 10)

    def echo_criterion_block(self, r0, c0, nr, nc):
        """the records [nr, nc, 10] of result cells [r0, r0 + nr) x [c0, c0 + nc)"""
        return self._map_block(lib().PvAmdCopyEchoCriterionBlock, r0, c0, nr, nc, 10)

    def echo_criterion_at(self, pos):
        """float32 [10] at an emitter position (the cell get_output reads); ten NaNs off the map"""
        return self._map_at(lib().PvAmdGetEchoCriterion, pos, record=PvAmdEchoCriterion)

    def compute_lateral_fraction(self):
        """early lateral energy fraction and early-sound direction (LATERAL_FRACTION_NAMES) of the last completed run: the
        velocity recurrence through the 80 ms window of every reached cell, on the device; returns the pass's device time in
        milliseconds"""
        return self._map_ms(lib().PvAmdComputeLateralFraction)

    def lateral_fraction(self):
        """float32 [gx, gy, 11] (LATERAL_FRACTION_NAMES); NaN where the cell has no onset in the run they were computed for, and
        in lf / dir_x / dir_y where the early flux is zero"""
        return self._map_all(lib().PvAmdCopyLateralFraction, 11)

    def lateral_fraction_block(self, r0, c0, nr, nc):
        """the records [nr, nc, 11] of result cells [r0, r0 + nr) x [c0, c0 + nc)"""
        return self._map_block(lib().PvAmdCopyLateralFractionBlock, r0, c0, nr, nc, 11)

    def lateral_fraction_at(self, pos):
        """float32 [11] at an emitter position (the cell get_output reads); eleven NaNs off the map"""
        return self._map_at(lib().PvAmdGetLateralFraction, pos, record=PvAmdLateralFraction)

    def set_echogram(self, slot_seconds, n_slots):
        """the time slots compute_echogram sums into: n_slots (at most ECHOGRAM_MAX_SLOTS) of (int)(slot_seconds * fs) steps each,
        from every cell's own onset on; n_slots = 0 clears them and frees the device storage"""
        _check(lib().PvAmdSetEchogram(self._h, float(slot_seconds), int(n_slots)))

    def echogram_slots(self):
        """(n, slot_seconds, slot_steps): the slots as set; (0, 0.0, 0) when none are"""
        sec, steps = C.c_float(0.0), C.c_int(0)
        n = lib().PvAmdGetEchogramSlots(self._h, C.byref(sec), C.byref(steps))
        if n < 0:
            raise PlaneverbError(last_error())
        return n, sec.value, steps.value

    def compute_echogram(self):
        """directional echogram of the last completed run at the slots of set_echogram: energy p^2 and flux p vx, p vy of
        every reached cell per slot, the velocity by the stencil's recurrence, on the device; returns the pass's device time in
        milliseconds"""
        return self._map_ms(lib().PvAmdComputeEchogram)

    def echogram(self):
        """float32 [gx, gy, 1 + 3 n]: n = the steps summed, then e, ix, iy of each slot; NaN where the cell has no onset in the
        run they were computed for.  (ix, iy) is the direction slot j's sound travels in, neither normalised nor negated"""
        return self._map_all(lib().PvAmdCopyEchogram, 1 + 3 * self.echogram_slots()[0])

    def echogram_block(self, r0, c0, nr, nc):
        """the records [nr, nc, 1 + 3 n] of result cells [r0, r0 + nr) x [c0, c0 + nc)"""
        return self._map_block(lib().PvAmdCopyEchogramBlock, r0, c0, nr, nc, 1 + 3 * self.echogram_slots()[0])

    def echogram_at(self, pos):
        """float32 [1 + 3 n] at an emitter position (the cell get_output reads); NaNs off the map"""
        return self._map_at(lib().PvAmdGetEchogram, pos, 1 + 3 * self.echogram_slots()[0])

    def set_lobe_windows(self, edges=None):
        """the time windows compute_lobes sums into, by their edges in seconds after every cell's own onset (at most
        LOBES_MAX_EDGES, step counts (int)(edge * fs) strictly increasing from 1 on); None or empty restores the default,
        10 ms and 80 ms: direct, early, late"""
        e, ep = _lobe_edges(edges)
        _check(lib().PvAmdSetLobeWindows(self._h, ep, int(e.size)))

    def lobe_windows(self):
        """(edges_seconds, edge_steps): the window edges in force, float32 [nE] and int32 [nE]; nW = nE + 1 windows"""
        sec, steps = np.zeros(LOBES_MAX_EDGES, np.float32), np.zeros(LOBES_MAX_EDGES, np.int32)
        n = lib().PvAmdGetLobeWindows(self._h, _f(sec), steps.ctypes.data_as(C.POINTER(C.c_int)))
        if n < 0:
            raise PlaneverbError(last_error())
        return sec[:n].copy(), steps[:n].copy()

    def _lobe_floats(self):
        return 1 + 5 * (len(self.lobe_windows()[0]) + 1)

    def compute_lobes(self):
        """directional energy lobes of the last completed run for the windows of set_lobe_windows: the energy p^2 of every
        reached cell per window and its split over the travel directions +x, -x, +y, -y, the velocity by the stencil's recurrence,
        on the device; returns the pass's device time in milliseconds"""
        return self._map_ms(lib().PvAmdComputeLobes)

    def lobes(self):
        """float32 [gx, gy, 1 + 5 nW]: n = the steps of the response, then LOBE_NAMES (e, xp, xn, yp, yn) of each window; NaN
        where the cell has no onset in the run they were computed for.  xp is the energy that travels towards +x at the cell"""
        return self._map_all(lib().PvAmdCopyLobes, self._lobe_floats())

    def lobes_block(self, r0, c0, nr, nc):
        """the records [nr, nc, 1 + 5 nW] of result cells [r0, r0 + nr) x [c0, c0 + nc)"""
        return self._map_block(lib().PvAmdCopyLobesBlock, r0, c0, nr, nc, self._lobe_floats())

    def lobes_at(self, pos):
        """float32 [1 + 5 nW] at an emitter position (the cell get_output reads); NaNs off the map"""
        return self._map_at(lib().PvAmdGetLobes, pos, self._lobe_floats())

    def set_bands(self, hz, fraction=1):
        """the band centres (Hz, at most BANDS_MAX) compute_band_metrics filters into, octaves (fraction 1) or third octaves
        (fraction 3), each with its upper edge below fs / 2; an empty list clears them and frees the device storage"""
        h = np.ascontiguousarray(hz, np.float32).reshape(-1)
        _check(lib().PvAmdSetBands(self._h, _f(h) if h.size else None, int(h.size), int(fraction)))

    def bands(self):
        """(float32 [n], fraction): the band centres as set"""
        out = np.empty(BANDS_MAX, np.float32)
        fr = C.c_int(1)
        n = lib().PvAmdGetBands(self._h, _f(out), BANDS_MAX, C.byref(fr))
        if n < 0:
            raise PlaneverbError(last_error())
        return out[:n].copy(), fr.value

    def band_coefs(self):
        """float32 [n, 10]: the filter coefficients the device uses (host_band_coefs of the solver's fs)"""
        out = np.empty((len(self.bands()[0]), 10), np.float32)
        _check(lib().PvAmdGetBandCoefs(self._h, _f(out)))
        return out

    def compute_band_metrics(self):
        """decay times and clarity per band (BAND_METRIC_NAMES) of the last completed run at the bands of set_bands, on the
        device; returns the device time of the passes in milliseconds"""
        return self._map_ms(lib().PvAmdComputeBandMetrics)

    def band_metrics(self):
        """float32 [gx, gy, n, 12] (BAND_METRIC_NAMES); NaN where the cell has no onset in the run they were computed for"""
        return self._map_all(lib().PvAmdCopyBandMetrics, len(self.bands()[0]), 12)

    def band_metrics_block(self, r0, c0, nr, nc):
        """the records [nr, nc, n, 12] of result cells [r0, r0 + nr) x [c0, c0 + nc)"""
        return self._map_block(lib().PvAmdCopyBandMetricsBlock, r0, c0, nr, nc, len(self.bands()[0]), 12)

    def band_metrics_at(self, pos):
        """float32 [n, 12] at an emitter position (the cell get_output reads); NaNs off the map"""
        return self._map_at(lib().PvAmdGetBandMetrics, pos, len(self.bands()[0]), 12)

    def set_modulation_frequencies(self, hz=None):
        """the 14 modulation frequencies (Hz, each in [0, fs / 2]) compute_modulation evaluates; None restores the default series
        (MODULATION_DEFAULT_HZ)"""
        h = _hz14(hz)
        _check(lib().PvAmdSetModulationFrequencies(self._h, _f(h) if h is not None else None))

    def modulation_frequencies(self):
        """float32 [14]: the modulation frequencies in use"""
        out = np.empty(MODULATION_FREQS, np.float32)
        _check(lib().PvAmdGetModulationFrequencies(self._h, _f(out)))
        return out

    def compute_modulation(self):
        """the modulation transfer function and index per band of set_bands of the last completed run, on the device; returns the
        device time of the passes in milliseconds"""
        return self._map_ms(lib().PvAmdComputeModulation)

    def modulation(self):
        """float32 [gx, gy, n, 15] (m at the 14 modulation frequencies, then mti); NaN where the cell has no onset in the run they
        were computed for"""
        return self._map_all(lib().PvAmdCopyModulation, len(self.bands()[0]), MODULATION_FREQS + 1)

    def modulation_block(self, r0, c0, nr, nc):
        """the records [nr, nc, n, 15] of result cells [r0, r0 + nr) x [c0, c0 + nc)"""
        return self._map_block(lib().PvAmdCopyModulationBlock, r0, c0, nr, nc, len(self.bands()[0]), MODULATION_FREQS + 1)

    def modulation_at(self, pos):
        """float32 [n, 15] at an emitter position (the cell get_output reads); NaNs off the map"""
        return self._map_at(lib().PvAmdGetModulation, pos, len(self.bands()[0]), MODULATION_FREQS + 1)

    def set_spectrum_bins(self, hz):
        """the frequencies (Hz, at most SPECTRUM_MAX_BINS, each in [0, fs / 2]) compute_spectrum evaluates; an empty list clears
        them and frees the device storage"""
        h = np.ascontiguousarray(hz, np.float32).reshape(-1)
        _check(lib().PvAmdSetSpectrumBins(self._h, _f(h) if h.size else None, int(h.size)))

    def spectrum_bins(self):
        """float32 [n]: the bins as set"""
        out = np.empty(SPECTRUM_MAX_BINS, np.float32)
        n = lib().PvAmdGetSpectrumBins(self._h, _f(out), SPECTRUM_MAX_BINS)
        if n < 0:
            raise PlaneverbError(last_error())
        return out[:n].copy()

    def spectrum_source(self):
        """float32 [n, 3]: sre, sim, spow of the run's pulse at every bin (what the levels are relative to)"""
        out = np.empty((len(self.spectrum_bins()), 3), np.float32)
        _check(lib().PvAmdGetSpectrumSource(self._h, _f(out)))
        return out

    def compute_spectrum(self):
        """transfer functions of the last completed run at the bins of set_spectrum_bins, on the device; returns the device
        time of the passes in milliseconds"""
        return self._map_ms(lib().PvAmdComputeSpectrum)

    def spectrum(self):
        """float32 [gx, gy, n, 3] (re, im, level in dB; X(f) = re - i im); NaN where the cell has no onset in the run they were
        computed for"""
        return self._map_all(lib().PvAmdCopySpectrum, len(self.spectrum_bins()), 3)

    def spectrum_block(self, r0, c0, nr, nc):
        """the records [nr, nc, n, 3] of result cells [r0, r0 + nr) x [c0, c0 + nc)"""
        return self._map_block(lib().PvAmdCopySpectrumBlock, r0, c0, nr, nc, len(self.spectrum_bins()), 3)

    def spectrum_at(self, pos):
        """float32 [n, 3] at an emitter position (the cell get_output reads); NaNs off the map"""
        return self._map_at(lib().PvAmdGetSpectrum, pos, len(self.spectrum_bins()), 3)

    def set_waterfall(self, hz, slice_seconds=0.0, n_slices=0):
        """the bins (Hz, at most WATERFALL_MAX_BINS, each in [0, fs / 2]) and the slices (n_slices of slice_seconds each, at most
        WATERFALL_MAX_SLICES) compute_waterfall evaluates; uploads the tables; an empty list clears the setting and frees the
        device storage"""
        h = np.ascontiguousarray(hz, np.float32).reshape(-1)
        _check(lib().PvAmdSetWaterfall(self._h, _f(h) if h.size else None, int(h.size), float(slice_seconds), int(n_slices)))

    def waterfall_setting(self):
        """(hz float32 [n], slice_seconds, slice_steps, n_slices) as set; None without a setting"""
        hz = np.empty(WATERFALL_MAX_BINS, np.float32)
        sec, steps, m = C.c_float(0.0), C.c_int(0), C.c_int(0)
        n = lib().PvAmdGetWaterfall(self._h, _f(hz), WATERFALL_MAX_BINS, C.byref(sec), C.byref(steps), C.byref(m))
        if n < 0:
            raise PlaneverbError(last_error())
        return (hz[:n].copy(), sec.value, steps.value, m.value) if n else None

    def compute_waterfall(self, positions=None):
        """the waterfalls of the last completed run at `positions` ([N, 3], mapped to cells as set_output_queries maps them) --
        on a sparse-emitter solver positions = None: the receivers are the emitters set_emitters kept --, on the device; returns
        the device time of the pass in milliseconds"""
        ms = C.c_float(0.0)
        if positions is None:
            _check(lib().PvAmdComputeWaterfall(self._h, None, 0, C.byref(ms)))
            self._waterfall_count = len(self.emitter_cells())
        else:
            xyz = np.ascontiguousarray(positions, np.float32).reshape(-1, 3)
            _check(lib().PvAmdComputeWaterfall(self._h, _f(xyz) if xyz.size else None, int(xyz.shape[0]), C.byref(ms)))
            self._waterfall_count = int(xyz.shape[0])
        return ms.value

    def waterfall(self, count=None):
        """the records compute_waterfall left: onset [N] and slices [N] (the onset step, the slices that start inside the run),
        response [N, n, 2] (R, I of slice 0: X(f) = R - i I) and level [N, m, n] (dB re the source, slice-major); NaN rows for
        receivers without an onset in that run.  count: the computed receivers (default: those of the last compute_waterfall of
        this object -- the kept emitters on a sparse-emitter solver)"""
        st = self.waterfall_setting()
        if st is None:
            _check(lib().PvAmdCopyWaterfall(self._h, _f(np.empty(1, np.float32)), 0))  # (raises with the library's words)
        n, m = len(st[0]), st[3]
        if count is None:
            count = getattr(self, "_waterfall_count", 0)
        rec = np.empty((int(count), 2 + 2 * n + m * n), np.float32)
        _check(lib().PvAmdCopyWaterfall(self._h, _f(rec), int(count)))
        return _waterfall_dict(rec, n, m)

    def set_arrays(self, arrays, interp=ARRAY_LAGRANGE3):
        """the source arrays compute_arrays mixes: a list of arrays, each a list of members (pos, gain, delay_seconds) with pos =
        (x, y, z); at most ARRAYS_MAX arrays of at most ARRAY_MEMBERS_MAX members; an empty list clears the setting and frees the
        device storage"""
        count = np.array([len(a) for a in arrays], np.int32)
        rows = [[float(p[0]), float(p[1]), float(p[2]), float(g), float(d)] for a in arrays for (p, g, d) in a]
        mem = np.ascontiguousarray(rows, np.float32).reshape(-1, 5)
        _check(lib().PvAmdSetArrays(self._h, _ip(count) if count.size else None, int(count.size), _f(mem) if mem.size else None, int(interp)))

    def arrays(self):
        """(counts int32 [n_arrays], interp) as set; None without a setting"""
        count, interp = np.zeros(ARRAYS_MAX, np.int32), C.c_int(0)
        n = lib().PvAmdGetArrays(self._h, _ip(count), ARRAYS_MAX, C.byref(interp))
        if n < 0:
            raise PlaneverbError(last_error())
        return (count[:n].copy(), interp.value) if n else None

    def array_taps(self, i):
        """the expanded taps of array i in the order its response takes them: (member int32 [n], delay_steps int32 [n], weight
        float32 [n])"""
        cap = 4 * ARRAY_MEMBERS_MAX
        m, d, w = np.zeros(cap, np.int32), np.zeros(cap, np.int32), np.zeros(cap, np.float32)
        n = lib().PvAmdGetArrayTaps(self._h, int(i), _ip(m), _ip(d), _f(w), cap)
        if n < 0:
            raise PlaneverbError(last_error())
        return m[:n].copy(), d[:n].copy(), w[:n].copy()

    def set_array_records(self, time_kinds, spectral_kinds=0):
        """the record kinds compute_arrays computes for every array: a mask of QREC_ROOM_METRICS, QREC_DECAY_TIMES,
        QREC_ECHO_CRITERION and a mask of QSPEC_*; both 0 selects none"""
        _check(lib().PvAmdSetArrayRecords(self._h, int(time_kinds), int(spectral_kinds)))

    def array_record_kinds(self):
        """(time kinds, spectral kinds)"""
        t, f = C.c_uint(0), C.c_uint(0)
        _check(lib().PvAmdGetArrayRecordKinds(self._h, C.byref(t), C.byref(f)))
        return int(t.value), int(f.value)

    def compute_arrays(self):
        """mix, onsets and the selected records of the arrays for the last completed run, on the device; returns the device time
        in milliseconds"""
        ms = C.c_float(0.0)
        _check(lib().PvAmdComputeArrays(self._h, C.byref(ms)))
        return ms.value

    def array_response(self, i):
        """float32 [T]: the response of array i as compute_arrays left it"""
        out = np.empty(self.T, np.float32)
        _check(lib().PvAmdCopyArrayResponse(self._h, int(i), _f(out)))
        return out

    def array_onsets(self):
        """float32 [n_arrays]: the onset step of every response, FLT_MAX where it has none"""
        st = self.arrays()
        n = len(st[0]) if st else 0
        out = np.empty(max(n, 1), np.float32)
        _check(lib().PvAmdGetArrayOnsets(self._h, _f(out), n))
        return out[:n]

    def array_records(self, kind, spectral=False):
        """float32 [n_arrays, floats] of ONE selected kind (QSPEC_* with spectral=True): row a is PvAmdHost<Kind> of array a's
        response with its onset, NaNs where it has none; the layout of emitter_records"""
        fam = 1 if spectral else 0
        floats = lib().PvAmdArrayRecordFloats(self._h, fam, int(kind))
        if floats < 0:
            raise PlaneverbError(last_error())
        st = self.arrays()
        n = len(st[0]) if st else 0
        out = np.empty((max(n, 1), floats), np.float32)
        _check(lib().PvAmdGetArrayRecords(self._h, fam, int(kind), _f(out), n))
        return out[:n]

    def set_auralisation(self, rate, zero_crossings=16, beta=9.0):
        """the audio rate compute_aural_responses resamples to (1000 .. 384000 samples per second) and the Kaiser-windowed sinc
        it uses (zero crossings per side at the lower rate, the window's beta); builds and uploads the tables; rate = 0 clears
        the setting and frees the device storage"""
        _check(lib().PvAmdSetAuralisation(self._h, int(rate), int(zero_crossings), float(beta)))

    def auralisation_setting(self):
        """(rate, zero_crossings, beta, L, K) as set, with the response length L in output samples and the taps per sample K;
        None without a setting"""
        rate, z, beta, L, K = C.c_int(0), C.c_int(0), C.c_float(0.0), C.c_int(0), C.c_int(0)
        if lib().PvAmdGetAuralisation(self._h, C.byref(rate), C.byref(z), C.byref(beta), C.byref(L), C.byref(K)) < 0:
            if last_error().startswith("aural: no setting"):
                return None
            raise PlaneverbError(last_error())
        return rate.value, z.value, beta.value, L.value, K.value

    def _aural_shape(self):
        st = self.auralisation_setting()
        if st is None:
            raise PlaneverbError("aural: no setting (PvAmdSetAuralisation)")
        return st[3], st[4]

    def aural_taps(self):
        """the resampling tables as uploaded: (first int32 [L], w float32 [L, K])"""
        L, K = self._aural_shape()
        first, w = np.empty(L, np.int32), np.empty((L, K), np.float32)
        if lib().PvAmdGetAuralTaps(self._h, _ip(first), _f(w), L) < 0:
            raise PlaneverbError(last_error())
        return first, w

    def compute_aural_responses(self, positions=None, source=AURAL_RECEIVERS):
        """the audio-rate responses of the last completed run, on the device: at `positions` ([N, 3], mapped to cells as
        set_output_queries maps them); with positions = None on a sparse-emitter solver of the emitters set_emitters kept; with
        source = AURAL_ARRAYS of the array responses compute_arrays left.  Returns the device time in milliseconds"""
        ms = C.c_float(0.0)
        if positions is None:
            _check(lib().PvAmdComputeAuralResponses(self._h, int(source), None, 0, C.byref(ms)))
            if source == AURAL_ARRAYS:
                st = self.arrays()
                self._aural_count = len(st[0]) if st else 0
            else:
                self._aural_count = len(self.emitter_cells())
        else:
            xyz = np.ascontiguousarray(positions, np.float32).reshape(-1, 3)
            _check(lib().PvAmdComputeAuralResponses(self._h, int(source), _f(xyz) if xyz.size else None, int(xyz.shape[0]), C.byref(ms)))
            self._aural_count = int(xyz.shape[0])
        return ms.value

    def aural_response(self, r):
        """float32 [L]: the response of receiver r at the audio rate, n = 0 the emission"""
        out = np.empty(self._aural_shape()[0], np.float32)
        _check(lib().PvAmdCopyAuralResponse(self._h, int(r), _f(out)))
        return out

    def set_aural_form(self, form):
        """the convolution kernel auralise launches: AURAL_TILED (the default) or AURAL_PLAIN; the same bits either way"""
        _check(lib().PvAmdSetAuralForm(self._h, int(form)))

    def auralise(self, signals, route, gain=None):
        """convolve the responses with dry signals and mix, on the device: signals float32 [n_signals, N] (or [N]) at the set rate,
        route[r] the signal receiver r renders or -1, gain[r] its weight in the mix (default 1).  Returns the device time in
        milliseconds; the outputs are N + L - 1 samples long"""
        x = np.ascontiguousarray(signals, np.float32)
        x = x.reshape(1, -1) if x.ndim == 1 else x
        rt = np.ascontiguousarray(route, np.int32).reshape(-1)
        g = np.ones(rt.size, np.float32) if gain is None else np.ascontiguousarray(gain, np.float32).reshape(-1)
        count = getattr(self, "_aural_count", None)  # (None: no responses were computed through this object; the library says so)
        if count is not None and (rt.size != count or g.size != count):
            raise ValueError("route and gain take one entry per receiver of compute_aural_responses (%d)" % count)
        ms = C.c_float(0.0)
        _check(lib().PvAmdAuralise(self._h, _f(x) if x.size else None, int(x.shape[0]), int(x.shape[1]), _ip(rt) if rt.size else None,
                                   _f(g) if g.size else None, C.byref(ms)))
        self._aural_m = int(x.shape[1]) + self._aural_shape()[0] - 1
        return ms.value

    def aural_output(self, r):
        """float32 [N + L - 1]: what receiver r renders, zeros where it is not routed"""
        out = np.empty(max(getattr(self, "_aural_m", 0), 1), np.float32)
        _check(lib().PvAmdCopyAuralOutput(self._h, int(r), _f(out)))
        return out

    def aural_mix(self):
        """float32 [N + L - 1]: the gain-weighted sum of the routed receivers' outputs"""
        out = np.empty(max(getattr(self, "_aural_m", 0), 1), np.float32)
        _check(lib().PvAmdCopyAuralMix(self._h, _f(out)))
        return out

    def set_zones(self, labels, n_zones=None):
        """the zones zone_stats reduces over: labels = uint8 [gx, gy], 0 = no zone, 1 .. n_zones (at most ZONES_MAX; None: the
        largest label), kept on the device across runs and geometry changes; labels = None clears them"""
        if labels is None:
            _check(lib().PvAmdSetZones(self._h, None, 0))
            return
        lab, n = _zone_labels(labels, n_zones)
        if lab.shape != (self.gx, self.gy):
            raise ValueError("set_zones: labels [gx, gy]")
        _check(lib().PvAmdSetZones(self._h, lab.ctypes.data_as(C.POINTER(C.c_ubyte)), n))

    def zones(self):
        """(labels uint8 [gx, gy], n_zones) as set; (None, 0) when no zones are set"""
        lab = np.zeros((self.gx, self.gy), np.uint8)
        n = C.c_int(0)
        _check(lib().PvAmdGetZones(self._h, lab.ctypes.data_as(C.POINTER(C.c_ubyte)), C.byref(n)))
        return (lab, n.value) if n.value else (None, 0)

    def _zone_width(self, kind):
        k = _map_kind(kind)
        planes = lib().PvAmdZoneStatPlanes(self._h, k)
        if planes < 0:
            raise PlaneverbError(last_error())
        per = {PVA_MAP_BAND_METRICS: 12, PVA_MAP_MODULATION: MODULATION_FREQS + 1, PVA_MAP_SPECTRUM: 3}.get(k)
        return k, planes, ((planes // per, per) if per else (planes,))

    def zone_stats(self, kind, with_ms=False):
        """PvAmdComputeZoneStats: the statistics of the computed map of `kind` (a name of MAP_KIND_NAMES or a PVA_MAP_* constant)
        over the zones of set_zones, reduced on the device -- a structured array (ZONE_STAT_DTYPE) of shape [n_zones, *width],
        width as the kind's map has it; with_ms: (records, device milliseconds)"""
        k, planes, width = self._zone_width(kind)
        nz = C.c_int(0)
        _check(lib().PvAmdGetZones(self._h, None, C.byref(nz)))
        n = nz.value
        out = np.zeros((max(n, 1), planes), ZONE_STAT_DTYPE)
        ms = C.c_float(0.0)
        got = lib().PvAmdComputeZoneStats(self._h, k, out.ctypes.data_as(_vp), out.size, C.byref(ms))
        if got < 0:
            raise PlaneverbError(last_error())
        out = out[:n].reshape((n,) + width)
        return (out, ms.value) if with_ms else out

    def zone_decay(self, align="absolute", curves=False, with_ms=False):
        """PvAmdComputeZoneDecay: the ensemble decay curve of every zone of set_zones over the last completed run -- the squared
        histories of the zone's reached cells summed on the device, slot j = t ("absolute") or t - onset ("onset") -- and EDT, T20
        and T30 read off it: records [n_zones] of ZONE_DECAY_DTYPE; curves: (records, etc, edc), float64 [n_zones, T] each;
        with_ms: the device milliseconds appended"""
        nz = C.c_int(0)
        lib().PvAmdGetZones(self._h, None, C.byref(nz))  # (a handle it refuses has no zones: the call below says why, in its own words)
        n = nz.value
        out = np.zeros(max(n, 1), ZONE_DECAY_DTYPE)
        etc = np.zeros((max(n, 1), self.T)) if curves else None
        edc = np.zeros((max(n, 1), self.T)) if curves else None
        ms = C.c_float(0.0)
        got = lib().PvAmdComputeZoneDecay(self._h, _zone_decay_align(align), out.ctypes.data_as(_vp), out.size,
                                          etc.ctypes.data_as(_dp) if curves else None, edc.ctypes.data_as(_dp) if curves else None,
                                          C.byref(ms))
        if got < 0:
            raise PlaneverbError(last_error())
        res = (out[:n],) + ((etc[:n], edc[:n]) if curves else ()) + ((ms.value,) if with_ms else ())
        return res[0] if len(res) == 1 else res

    def set_zone_curves(self, on):
        """PvAmdSetZoneCurves (sparse-emitter solvers, zones set): every following run accumulates the "absolute" curves of the
        zones on the device, off the ring, and zone_decay("absolute") reads them; False stops it and frees the buffers"""
        _check(lib().PvAmdSetZoneCurves(self._h, 1 if on else 0))

    def zone_curves(self):
        """PvAmdGetZoneCurves: True while set_zone_curves(True) holds"""
        on = C.c_int(0)
        _check(lib().PvAmdGetZoneCurves(self._h, C.byref(on)))
        return bool(on.value)

    def set_zone_maps(self, kinds):
        """PvAmdSetZoneMaps (sparse-emitter solvers, zones set): every following run accumulates the room-metrics (ZMAP_ROOM_METRICS)
        and / or spectrum (ZMAP_SPECTRUM; bins set) records of every labelled cell on the device, off the ring; room_metrics*,
        spectrum* and zone_stats of the two kinds then read that map (unlabelled cells: NaN).  0 deselects and frees"""
        _check(lib().PvAmdSetZoneMaps(self._h, int(kinds)))

    def zone_maps(self):
        """PvAmdGetZoneMaps: the kinds set_zone_maps holds"""
        k = C.c_uint(0)
        _check(lib().PvAmdGetZoneMaps(self._h, C.byref(k)))
        return int(k.value)

    def zone_decay_chunk_slots(self):
        """PvAmdZoneDecayChunkSlots: the time slots zone_decay deals per pair of launches under the current zones"""
        n = lib().PvAmdZoneDecayChunkSlots(self._h)
        if n < 0:
            raise PlaneverbError(last_error())
        return n

    def zone_band_decay(self, align="absolute", curves=False, with_ms=False):
        """PvAmdComputeZoneBandDecay: the ensemble decay curve of every zone of set_zones PER BAND of set_bands over the last
        completed run -- the band-filtered histories of the zone's reached cells squared and summed on the device -- with EDT, T20,
        T30 and the clarity (c50, c80, d50, ts) read off it: records [n_zones, n_bands] of ZONE_BAND_DECAY_DTYPE; curves: (records,
        etc, edc), float64 [n_zones, n_bands, T] each; with_ms: the device milliseconds appended"""
        nz, fr = C.c_int(0), C.c_int(1)
        lib().PvAmdGetZones(self._h, None, C.byref(nz))  # (a handle it refuses has no zones: the call below says why, in its own words)
        hz = np.empty(BANDS_MAX, np.float32)
        n, nb = nz.value, max(lib().PvAmdGetBands(self._h, _f(hz), BANDS_MAX, C.byref(fr)), 0)
        out = np.zeros((max(n, 1), max(nb, 1)), ZONE_BAND_DECAY_DTYPE)
        etc = np.zeros((max(n, 1), max(nb, 1), self.T)) if curves else None
        edc = np.zeros((max(n, 1), max(nb, 1), self.T)) if curves else None
        ms = C.c_float(0.0)
        got = lib().PvAmdComputeZoneBandDecay(self._h, _zone_decay_align(align), out.ctypes.data_as(_vp), n * nb,
                                              etc.ctypes.data_as(_dp) if curves else None,
                                              edc.ctypes.data_as(_dp) if curves else None, C.byref(ms))
        if got < 0:
            raise PlaneverbError(last_error())
        res = (out[:n, :nb],) + ((etc[:n, :nb], edc[:n, :nb]) if curves else ()) + ((ms.value,) if with_ms else ())
        return res[0] if len(res) == 1 else res

    def zone_band_decay_chunk(self):
        """PvAmdZoneBandDecayChunk: (chunks, slots, bands) -- the chunks of (zone, band) pairs zone_band_decay takes under the
        current zones and bands, the time slots of a chunk (T: time is never cut) and the bands of a chunk"""
        sl, bd = C.c_int(0), C.c_int(0)
        n = lib().PvAmdZoneBandDecayChunk(self._h, C.byref(sl), C.byref(bd))
        if n < 0:
            raise PlaneverbError(last_error())
        return n, sl.value, bd.value

    def pulse(self):
        """float32 [T]: the pulse table of a run (T = the run's steps; zero past the grid's own table)"""
        out = np.zeros(max(self.T, self._pulse_len), np.float32)  # (PvAmdCopyPulse writes the grid's own table)
        _check(lib().PvAmdCopyPulse(self._h, _f(out)))
        return out[:self.T].copy()

    def material(self):
        shp = (self.gx + 1, self.gy + 1)
        beta = np.empty(shp, np.uint8)
        R = np.empty(shp, np.float32)
        _check(lib().PvAmdCopyMaterial(self._h, beta.ctypes.data_as(C.POINTER(C.c_ubyte)), _f(R)))
        return beta, R
