"""ctypes binding of the MI355X solver library (``csrc/librmpc_hip.so``).

This is the thin host layer above the C ABI declared in ``include/rmpc.h``;
it plays the role ``forcespro.nlp.Solver`` plays for the reference planner
(``robotmpcs/planner/mpcPlanner.py:73,262``).  There is no CPU fallback: if the
library is missing or no HIP device is present the constructor raises.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _abi
from ._abi import RmpcError

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RMPC_LIB_PATH") or os.path.join(_HERE, "csrc", "librmpc_hip.so")


def _k(*names):
    """the values of the header's RMPC_<name> macros"""
    return tuple(_abi.constants["RMPC_" + n] for n in names)


MAX_JOINTS, MAX_LINKS, MAX_PAIRS, MAX_MODULES, NV_MAX = _k("MAX_JOINTS", "MAX_LINKS", "MAX_PAIRS", "MAX_MODULES", "NV_MAX")
MAX_XROWS, NUM_KERNELS = _k("MAX_XROWS", "NUM_KERNELS")

# The structs of include/rmpc.h, with the header's field names (_abi.py derives them from it).
RmpcDesc = _abi.structs["rmpc_desc"]                  # the model descriptor
RmpcScene = _abi.structs["rmpc_scene"]                # device pointers + broadcast weights
RetargetArgs = _abi.structs["rmpc_retarget"]          # the steady loop's goal hand-over, device pointers
LidarArgs = _abi.structs["rmpc_lidar"]                # one scan of B robots in a shared world, device pointers
LidarBodiesArgs = _abi.structs["rmpc_lidar_bodies"]   # the fleet's bodies a scan sees besides its world, device pointers
GridMarkArgs = _abi.structs["rmpc_grid_mark"]         # one scan of B robots added to the evidence grids, device pointers
ScanMatchArgs = _abi.structs["rmpc_scan_match"]       # one scan of B robots matched against the edge-distance table
ScanSearchArgs = _abi.structs["rmpc_scan_search"]     # rmpc_scan_match's fields, then the pyramid, workspace and outputs
TracksArgs = _abi.structs["rmpc_tracks"]              # one scan of B robots through the moving-obstacle tracker
TimedPlanArgs = _abi.structs["rmpc_timed_plan"]       # one prioritised space-time plan of B robots for G orders
TimedToursArgs = _abi.timed_tours_structs["rmpc_timed_tours"]     # the same through every robot's stops (rmpc_timed_tours.h)
TimedReplanArgs = _abi.timed_replan_structs["rmpc_timed_replan"]  # what a re-plan adds to it (rmpc_timed_replan.h)
TimedRepairArgs = _abi.timed_repair_structs["rmpc_timed_repair"]  # rmpc_timed_plan's members, then the repair's (rmpc_timed_repair.h)

# every symbol include/rmpc.h declares
EXPORTED_SYMBOLS = list(_abi.prototypes)
# and every symbol include/rmpc_grid_large.h declares
GRID_LARGE_SYMBOLS = list(_abi.large_prototypes)
# and every symbol include/rmpc_assign_opt.h declares
ASSIGN_OPT_SYMBOLS = list(_abi.assign_prototypes)
# and every symbol include/rmpc_tours.h declares
TOURS_SYMBOLS = list(_abi.tours_prototypes)
# and every symbol include/rmpc_timed_tours.h declares
TIMED_TOURS_SYMBOLS = list(_abi.timed_tours_prototypes)
# and every symbol include/rmpc_timed_replan.h declares
TIMED_REPLAN_SYMBOLS = list(_abi.timed_replan_prototypes)
# and every symbol include/rmpc_timed_repair.h declares
TIMED_REPAIR_SYMBOLS = list(_abi.timed_repair_prototypes)
# and every symbol include/rmpc_any_angle.h declares
ANY_ANGLE_SYMBOLS = list(_abi.any_angle_prototypes)
# and every symbol include/rmpc_corridor.h declares
CORRIDOR_SYMBOLS = list(_abi.corridor_prototypes)
# and every symbol include/rmpc_traffic.h declares
TRAFFIC_SYMBOLS = list(_abi.traffic_prototypes)
TrafficCostsArgs = _abi.traffic_structs["rmpc_traffic_costs"]     # the edge costs of the traffic-aware fields (rmpc_traffic.h)
# and every symbol include/rmpc_cbs.h declares
CBS_SYMBOLS = list(_abi.cbs_prototypes)
CbsArgs = _abi.cbs_structs["rmpc_cbs"]                            # one conflict-based search over the timed routes (rmpc_cbs.h)
# and every symbol include/rmpc_ecbs.h declares
ECBS_SYMBOLS = list(_abi.ecbs_prototypes)
EcbsArgs = _abi.ecbs_structs["rmpc_ecbs"]                         # rmpc_cbs's members, then the weight (rmpc_ecbs.h)

_lib = None


def source_files():
    """The files the library is built from (csrc/sources.txt), None when they are not shipped alongside."""
    root = os.path.dirname(_HERE)
    try:
        with open(os.path.join(_HERE, "csrc", "sources.txt")) as f:
            paths = [os.path.join(root, ln.strip()) for ln in f if ln.strip() and not ln.startswith("#")]
    except OSError:
        return None
    return paths if all(os.path.exists(p) for p in paths) else None


def _source_hash():
    """Hash of the sources next to the library (None when they are not shipped alongside)."""
    import hashlib
    paths = source_files()
    if paths is None:
        return None
    h = hashlib.sha256()
    for p in paths:
        with open(p, "rb") as f:
            h.update(f.read())
    return h.hexdigest()[:16]


def spec_source(desc: dict, name: str) -> str:
    """C++ text of the generated view of ``desc`` (``rmpc_spec_source``; needs no GPU)."""
    L = load_library()
    cd = make_desc(desc, 0)
    n = L.rmpc_spec_source(C.byref(cd), name.encode(), None, 0)
    if n < 0:
        raise RmpcError("rmpc_spec_source failed: " + L.rmpc_last_error().decode())
    buf = C.create_string_buffer(int(n))
    L.rmpc_spec_source(C.byref(cd), name.encode(), buf, n)
    return buf.value.decode()


def spec_for(desc: dict) -> str:
    """Name of the generated view ``rmpc_create`` would select for ``desc`` ("" = runtime row tables); no GPU needed."""
    cd = make_desc(desc, 0)
    return load_library().rmpc_spec_for(C.byref(cd)).decode()


def source_hash() -> str:
    """Hash embedded in the loaded library (``rmpc_source_hash()``)."""
    return load_library().rmpc_source_hash().decode()


def load_library(path: str = LIB_PATH):
    """dlopen the HIP library; raises ``RmpcError`` when it has not been built
    (``python -c 'import __graft_entry__ as g; g.build()'``)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise RmpcError(f"{path} not found: build the HIP extension first (__graft_entry__.build())")
    # PyTorch-ROCm wheels bundle their own libamdhip64 / libhsa-runtime64.  Two HIP
    # runtimes in one process cannot both open the GPU, so when torch is installed
    # it is imported first: the solver library (NEEDED libamdhip64.so.7) then binds
    # to the runtime torch already loaded and device pointers / streams are shared.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(path)
    # the declarations of include/rmpc.h, include/rmpc_grid_large.h, include/rmpc_assign_opt.h, include/rmpc_tours.h
    # include/rmpc_timed_tours.h, include/rmpc_timed_replan.h, include/rmpc_timed_repair.h, include/rmpc_any_angle.h,
    # include/rmpc_corridor.h, include/rmpc_traffic.h, include/rmpc_cbs.h and include/rmpc_ecbs.h, nothing else
    for name, (restype, argtypes) in (*_abi.prototypes.items(), *_abi.large_prototypes.items(),
                                      *_abi.assign_prototypes.items(), *_abi.tours_prototypes.items(),
                                      *_abi.timed_tours_prototypes.items(), *_abi.timed_replan_prototypes.items(),
                                      *_abi.timed_repair_prototypes.items(), *_abi.any_angle_prototypes.items(),
                                      *_abi.corridor_prototypes.items(), *_abi.traffic_prototypes.items(),
                                      *_abi.cbs_prototypes.items(), *_abi.ecbs_prototypes.items()):
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    if L.rmpc_desc_size() != C.sizeof(RmpcDesc):
        raise RmpcError("rmpc_desc layout mismatch between _lib.py and librmpc_hip.so")
    want = _source_hash()
    if os.environ.get("RMPC_ALLOW_STALE"):   # development aid (A/B against an older build); never set by product code
        want = None
    if want is not None and L.rmpc_source_hash().decode() != want:
        raise RmpcError("librmpc_hip.so is stale: built from other sources than the ones next to it "
                        f"({L.rmpc_source_hash().decode()} != {want}); run __graft_entry__.build()")
    _lib = L
    return L


def make_desc(d: dict, device: int = 0) -> RmpcDesc:
    """Descriptor dict (``rmpc_model.yaml``) -> ``rmpc_desc``."""
    o = RmpcDesc()
    o.struct_size = C.sizeof(RmpcDesc)
    o.device = int(device)
    o.robot = d["robot"]; o.N = d["N"]
    o.n, o.nx, o.nu, o.ns, o.npar = d["n"], d["nx"], d["nu"], d["ns"], d["npar"]
    o.dt = d["dt"]
    if len(d["module_kind"]) > MAX_MODULES or len(d["link_frame"]) > MAX_LINKS or \
            len(d["pair_frame"]) > MAX_PAIRS or len(d["joints"]) > MAX_JOINTS:
        raise RmpcError("descriptor exceeds the ABI's fixed capacities")
    o.n_modules = len(d["module_kind"])
    for i, k in enumerate(d["module_kind"]):
        o.module_kind[i] = k
    o.nobst = d["nobst"]
    o.n_links = len(d["link_frame"])
    for i, f in enumerate(d["link_frame"]):
        o.link_frame[i] = f
    o.n_pairs = len(d["pair_frame"])
    for i, (a, b) in enumerate(d["pair_frame"]):
        o.pair_frame[i][0] = a; o.pair_frame[i][1] = b
    o.end_frame = d["end_frame"]
    o.n_joints = len(d["joints"])
    for i, j in enumerate(d["joints"]):
        o.joint_type[i] = j["type"]; o.joint_dof[i] = j["dof"]
        for c in range(3):
            o.joint_xyz[i][c] = j["xyz"][c]; o.joint_axis[i][c] = j["axis"][c]
        for c in range(9):
            o.joint_rot[i][c] = j["rot"][c]
    for k in ("off_r_body", "off_obst", "off_lin", "off_lower", "off_upper", "off_lower_u", "off_upper_u",
              "off_lower_vel", "off_upper_vel", "off_wu", "off_goal", "off_wgoal", "off_wconstr", "off_ws",
              "has_goal", "has_avoid"):
        setattr(o, k, d[k])
    nv = d["nx"] + d["ns"] + d["nu"]
    for i in range(NV_MAX):
        o.lb[i] = float(d["lb"][i]) if i < nv else -np.inf
        o.ub[i] = float(d["ub"][i]) if i < nv else np.inf
    opt = d.get("options", {})
    o.max_iter = int(opt.get("max_iter", 200))
    o.tol_stat = float(opt.get("tol_stat", 1e-6)); o.tol_eq = float(opt.get("tol_eq", 1e-8))
    o.tol_ineq = float(opt.get("tol_ineq", 1e-8)); o.tol_comp = float(opt.get("tol_comp", 1e-6))
    o.mu0 = float(opt.get("mu0", 1.0))
    o.acc_iters = int(opt.get("acc_iters", 8)); o.acc_obj_tol = float(opt.get("acc_obj_tol", 1e-8))
    o.ls_max = int(opt.get("ls_max", 25))
    xrows = d.get("xrows", [])
    if len(xrows) > MAX_XROWS:
        raise RmpcError("more than %d described rows" % MAX_XROWS)
    o.n_xrows = len(xrows)
    for i, r in enumerate(xrows):
        o.xrow_mod[i], o.xrow_kind[i], o.xrow_a[i], o.xrow_b[i], o.xrow_poff[i] = (int(v) for v in r)
    return o


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _stream_arg(stream):
    """``stream``: an int / hipStream_t handle, or None = the stream the caller's torch ops run on
    (``torch.cuda.current_stream()``; the legacy null stream when torch is absent), so that the solver's
    kernels are ordered after the ops that produced the inputs and before the ops that read the outputs."""
    if stream is None:
        try:
            import torch
            if torch.cuda.is_available():
                stream = torch.cuda.current_stream().cuda_stream
        except ImportError:
            stream = 0
    return C.c_void_p(int(stream or 0))


def stream_handle(stream, device):
    """``stream`` (a raw handle), or when it is None that of the stream torch's ops run on on ``device`` -- the device of
    the call's tensors, which need not be the current one (``_stream_arg(None)`` asks the current device)."""
    import torch
    return stream if stream is not None else torch.cuda.current_stream(device).cuda_stream


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


WAVE_REDUCE_OPS = {"sum": 0, "max": 1, "min": 2, "many541": 3, "many102": 4}


def debug_wave_reduce(values, op: str, lpi: int, device: int = 0):
    """Test aid (``rmpc_debug_wave_reduce``): the kernels' whole-horizon reductions over ``lpi`` (32 or 64) consecutive
    lanes of one wavefront.  ``values`` [words][64] float64, at most 10 words per lane (``op``: "sum" / "max" / "min"
    reduce word 0; "many541" sums words 0 .. 4, takes the maxima of 5 .. 8 and the minimum of 9; "many102" sums word 0
    and takes the minima of words 1, 2, word 3 of the result being the maximum of the kernels' constant zero).  Returns
    (shuffle form, vector-move form), each [10][64]: every lane's result."""
    v = np.zeros((10, 64), dtype=np.float64)
    a = np.asarray(values, dtype=np.float64).reshape(-1, 64)
    v[:a.shape[0]] = a
    ref, new = np.empty_like(v), np.empty_like(v)
    L = load_library()
    if L.rmpc_debug_wave_reduce(int(device), int(lpi), WAVE_REDUCE_OPS[op], _dp(v), _dp(ref), _dp(new)) != 0:
        raise RmpcError("rmpc_debug_wave_reduce: " + L.rmpc_last_error().decode())
    return ref, new


def free_space_decomposition_device(points, seeds, planes_out, max_radius: float, stream=None):
    """points (B, P, 3), seeds (B, N, 3), planes_out (B, N, K, 4): contiguous fp64 device tensors.
    Device counterpart of ``FreeSpaceDecomposition.compute_constraints`` + ``asdict`` of the
    reference (``robotmpcs/utils/free_space_decomposition.py:79-116``) for B*N seeds at once."""
    L = load_library()
    B, P = int(points.shape[0]), int(points.shape[1])
    N, K = int(seeds.shape[1]), int(planes_out.shape[2])
    st = _stream_arg(stream)
    rc = L.rmpc_free_space_device(B, N, P, K, float(max_radius), C.c_void_p(points.data_ptr()),
                                  C.c_void_p(seeds.data_ptr()), C.c_void_p(planes_out.data_ptr()), st)
    if rc != 0:
        raise RmpcError("rmpc_free_space_device failed: " + L.rmpc_last_error().decode())


# status codes of the global planner (include/rmpc.h)
GRID_MAX_CELLS, GRID_OK, GRID_START_OCCUPIED, GRID_GOAL_OCCUPIED, GRID_OUTSIDE, GRID_TOO_LONG = _k(
    "GRID_MAX_CELLS", "GRID_OK", "GRID_START_OCCUPIED", "GRID_GOAL_OCCUPIED", "GRID_OUTSIDE", "GRID_TOO_LONG")
GRID_BAD_MAP, GRID_NO_FIXED_POINT, GRID_BAD_SEED = _k("GRID_BAD_MAP", "GRID_NO_FIXED_POINT", "GRID_BAD_SEED")
# limits of the assignment (include/rmpc.h)
ASSIGN_MAX_ROBOTS, ASSIGN_MAX_TARGETS = _k("ASSIGN_MAX_ROBOTS", "ASSIGN_MAX_TARGETS")
# limits of the scan match: the rays (include/rmpc.h) and nxy, nth (kMatchMaxN, csrc/rmpc_locate.hpp)
MATCH_MAX_RAYS, = _k("MATCH_MAX_RAYS")
MATCH_MAX_N = 15


def _grid_call(name, *args):
    L = load_library()
    rc = getattr(L, name)(*args)
    if rc != 0:
        raise RmpcError(name + " failed: " + L.rmpc_last_error().decode())


def _size_query(name, *ints):
    """a host-only size function of the library: its count, or RmpcError when it answers -1"""
    L = load_library()
    n = getattr(L, name)(*(int(v) for v in ints))
    if n < 0:
        raise RmpcError(name + " failed: " + L.rmpc_last_error().decode())
    return int(n)


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def grid_inflate_device(grid, out, cell: float, size_robot: float, threshold: float = 0.29, stream=None):
    """grid, out (H, W) contiguous fp64 device tensors: ``GlobalPlanner.get_enlarged_obstacles`` of the reference
    (globalPlanner.py:39-70) on the device."""
    H, W = int(grid.shape[0]), int(grid.shape[1])
    _grid_call("rmpc_grid_inflate_device", H, W, float(cell), float(size_robot), float(threshold), _ptr(grid), _ptr(out),
               _stream_arg(stream))


def grid_fields_device(grid, goal_cells, fields, status, movement: int = 8, occ_threshold: float = 0.8,
                       cost_factor: float = 3.0, sweeps=None, stream=None):
    """grid (H, W) fp64, goal_cells (G,) int32, fields (G, H, W) fp64, status (G,) int32, sweeps (G,) int32 or None:
    one cost-to-go field per goal (``rmpc_grid_fields_device``)."""
    H, W = int(grid.shape[0]), int(grid.shape[1])
    _grid_call("rmpc_grid_fields_device", H, W, _ptr(grid), int(goal_cells.shape[0]), _ptr(goal_cells), int(movement),
               float(occ_threshold), float(cost_factor), _ptr(fields), _ptr(status),
               None if sweeps is None else _ptr(sweeps), _stream_arg(stream))


def grid_paths_device(grid, fields, goal_cells, start_cell, goal_index, path, length, movement: int = 8,
                      occ_threshold: float = 0.8, cost_factor: float = 3.0, stream=None):
    """start_cell, goal_index (B,) int32, path (B, max_len) int32, length (B,) int32: descent of the fields
    (``rmpc_grid_paths_device``)."""
    H, W = int(grid.shape[0]), int(grid.shape[1])
    _grid_call("rmpc_grid_paths_device", H, W, _ptr(grid), int(fields.shape[0]), _ptr(fields), _ptr(goal_cells),
               int(start_cell.shape[0]), _ptr(start_cell), _ptr(goal_index), int(movement), float(occ_threshold),
               float(cost_factor), int(path.shape[1]), _ptr(path), _ptr(length), _stream_arg(stream))


def grid_fields_seeded_device(grid, seeds, fields, status, movement: int = 8, occ_threshold: float = 0.8,
                              cost_factor: float = 3.0, sweeps=None, stream=None):
    """grid (H, W) fp64, seeds (G, H, W) fp64 (+inf no source, >= 0 a source's start potential), fields (G, H, W) fp64,
    status (G,) int32, sweeps (G,) int32 or None: one field to the nearest source per seed grid
    (``rmpc_grid_fields_seeded_device``)."""
    H, W = int(grid.shape[0]), int(grid.shape[1])
    _grid_call("rmpc_grid_fields_seeded_device", H, W, _ptr(grid), int(seeds.shape[0]), _ptr(seeds), int(movement),
               float(occ_threshold), float(cost_factor), _ptr(fields), _ptr(status),
               None if sweeps is None else _ptr(sweeps), _stream_arg(stream))


# limits of the fields on large maps (include/rmpc_grid_large.h)
GRID_LARGE_MAX_CELLS, GRID_LARGE_MAX_SIDE, GRID_TILE = (
    _abi.large_constants["RMPC_" + n] for n in ("GRID_LARGE_MAX_CELLS", "GRID_LARGE_MAX_SIDE", "GRID_TILE"))


def grid_fields_large_device(grid, goal_cells, fields, status, movement: int = 8, occ_threshold: float = 0.8,
                             cost_factor: float = 3.0, visits=None, stream=None):
    """As ``grid_fields_device`` on maps up to ``GRID_LARGE_MAX_CELLS`` cells, the same fields bit for bit; visits (G,)
    int32 or None: the tile visits each field took (``rmpc_grid_fields_large_device``)."""
    H, W = int(grid.shape[0]), int(grid.shape[1])
    _grid_call("rmpc_grid_fields_large_device", H, W, _ptr(grid), int(goal_cells.shape[0]), _ptr(goal_cells),
               int(movement), float(occ_threshold), float(cost_factor), _ptr(fields), _ptr(status),
               None if visits is None else _ptr(visits), _stream_arg(stream))


def grid_fields_seeded_large_device(grid, seeds, fields, status, movement: int = 8, occ_threshold: float = 0.8,
                                    cost_factor: float = 3.0, visits=None, stream=None):
    """As ``grid_fields_seeded_device`` on maps up to ``GRID_LARGE_MAX_CELLS`` cells, the same fields bit for bit;
    visits (G,) int32 or None: the tile visits each field took (``rmpc_grid_fields_seeded_large_device``)."""
    H, W = int(grid.shape[0]), int(grid.shape[1])
    _grid_call("rmpc_grid_fields_seeded_large_device", H, W, _ptr(grid), int(seeds.shape[0]), _ptr(seeds),
               int(movement), float(occ_threshold), float(cost_factor), _ptr(fields), _ptr(status),
               None if visits is None else _ptr(visits), _stream_arg(stream))


def grid_descend_device(grid, fields, seeds, start_cell, field_index, path, length, movement: int = 8,
                        occ_threshold: float = 0.8, cost_factor: float = 3.0, stream=None):
    """start_cell, field_index (B,) int32, path (B, max_len) int32, length (B,) int32: descent of the seeded fields
    (G, H, W) to a source nothing undercuts, from a start cell that may be occupied (``rmpc_grid_descend_device``)."""
    H, W = int(grid.shape[0]), int(grid.shape[1])
    _grid_call("rmpc_grid_descend_device", H, W, _ptr(grid), int(fields.shape[0]), _ptr(fields), _ptr(seeds),
               int(start_cell.shape[0]), _ptr(start_cell), _ptr(field_index), int(movement), float(occ_threshold),
               float(cost_factor), int(path.shape[1]), _ptr(path), _ptr(length), _stream_arg(stream))


def grid_cells_device(pos, cells, H: int, W: int, x0: float, y0: float, cell: float, stream=None):
    """pos (B, stride >= 2) fp64 (e.g. xinit), cells (B,) int32: world positions to cells of the plain frame."""
    _grid_call("rmpc_grid_cells_device", int(pos.shape[0]), _ptr(pos), int(pos.stride(0)), int(H), int(W), float(x0),
               float(y0), float(cell), _ptr(cells), _stream_arg(stream))


def follow_path_device(path, length, idx, pos, goal, W: int, x0: float, y0: float, cell: float, threshold: float = 1.3,
                       stream=None):
    """path (B, max_len), length (B,), idx (B,) int32; pos (B, stride >= 2) fp64; goal (B, 3) fp64: one control step
    of ``GlobalPlanner.get_local_goal`` for every robot (``rmpc_follow_path_device``)."""
    _grid_call("rmpc_follow_path_device", int(path.shape[0]), _ptr(path), _ptr(length), int(path.shape[1]), _ptr(idx),
               _ptr(pos), int(pos.stride(0)), int(W), float(x0), float(y0), float(cell), float(threshold), _ptr(goal),
               _stream_arg(stream))


# the limit of the follower that looks ahead (include/rmpc_any_angle.h)
VISIBLE_MAX_REACH = _abi.any_angle_constants["RMPC_VISIBLE_MAX_REACH"]


def shorten_work_bytes(H: int, W: int) -> int:
    """The bytes of workspace ``grid_shorten_device`` needs on an (H, W) map: the header's RMPC_SHORTEN_WORK_BYTES."""
    return 4 * int(H) * ((int(W) + 31) // 32)


def grid_visible_device(grid, cell_from, cell_to, visible, occ_threshold: float = 0.8, stream=None):
    """grid (H, W) fp64; cell_from, cell_to, visible (P,) int32: 1 where the second cell is in line of sight of the
    first, 0 where not, -1 for a cell outside the map (``rmpc_grid_visible_device``, include/rmpc_any_angle.h)."""
    H, W = int(grid.shape[0]), int(grid.shape[1])
    _grid_call("rmpc_grid_visible_device", H, W, _ptr(grid), float(occ_threshold), int(cell_from.shape[0]), _ptr(cell_from),
               _ptr(cell_to), _ptr(visible), _stream_arg(stream))


def grid_shorten_device(grid, path, length, out, out_length, work, reach: int = 0, keep=None, src=None,
                        occ_threshold: float = 0.8, stream=None):
    """path, out (B, max_len) int32, length, out_length (B,) int32; keep, src (B, max_len) int32 or None; work: a
    contiguous device tensor of at least ``shorten_work_bytes(H, W)`` bytes: every route pulled tight by line of sight
    (``rmpc_grid_shorten_device``)."""
    H, W = int(grid.shape[0]), int(grid.shape[1])
    if tuple(out.shape) != tuple(path.shape) or any(t is not None and tuple(t.shape) != tuple(path.shape) for t in (keep, src)):
        raise ValueError("grid_shorten_device: out, keep and src must have the shape of path")
    if not work.is_contiguous() or work.numel() * work.element_size() < shorten_work_bytes(H, W):
        raise ValueError("grid_shorten_device: need a contiguous workspace of shorten_work_bytes(H, W) bytes")
    _grid_call("rmpc_grid_shorten_device", H, W, _ptr(grid), float(occ_threshold), int(path.shape[0]), _ptr(path),
               _ptr(length), int(path.shape[1]), int(reach), None if keep is None else _ptr(keep), _ptr(out),
               _ptr(out_length), None if src is None else _ptr(src), _ptr(work), _stream_arg(stream))


def follow_visible_device(path, length, idx, pos, goal, grid, x0: float, y0: float, cell: float, reach: int = 16,
                          look_ahead: float = 1.3, blocked=None, occ_threshold: float = 0.8, stream=None):
    """``follow_path_device`` with a look-ahead that sees: every robot's waypoint moves on to the farthest route cell
    within ``reach`` cells and ``look_ahead`` metres that is in line of sight on grid (H, W) fp64; blocked (B,) int32 or
    None: 1 where no cell qualified (``rmpc_follow_visible_device``)."""
    H, W = int(grid.shape[0]), int(grid.shape[1])
    _grid_call("rmpc_follow_visible_device", int(path.shape[0]), _ptr(path), _ptr(length), int(path.shape[1]), _ptr(idx),
               _ptr(pos), int(pos.stride(0)), H, W, _ptr(grid), float(occ_threshold), float(x0), float(y0), float(cell),
               int(reach), float(look_ahead), _ptr(goal), None if blocked is None else _ptr(blocked), _stream_arg(stream))


# the limit of the corridors' reach (include/rmpc_corridor.h)
CORRIDOR_MAX_REACH = _abi.corridor_constants["RMPC_CORRIDOR_MAX_REACH"]


def corridor_sums_bytes(H: int, W: int) -> int:
    """The bytes of the summed-area table ``grid_occ_sums_device`` writes for an (H, W) map: the header's
    RMPC_CORRIDOR_SUMS_BYTES."""
    return 4 * (int(H) + 1) * (int(W) + 1)


def grid_occ_sums_device(grid, sums, occ_threshold: float = 0.8, stream=None):
    """grid (H, W) fp64 -> sums (H + 1, W + 1) int32, contiguous: the summed-area table of the occupancy
    (``rmpc_grid_occ_sums_device``, include/rmpc_corridor.h)."""
    H, W = int(grid.shape[0]), int(grid.shape[1])
    if tuple(sums.shape) != (H + 1, W + 1) or sums.element_size() != 4 or not sums.is_contiguous() or not grid.is_contiguous():
        raise ValueError("grid_occ_sums_device: need a contiguous grid (H, W) and a contiguous int32 sums (H + 1, W + 1)")
    _grid_call("rmpc_grid_occ_sums_device", H, W, _ptr(grid), float(occ_threshold), _ptr(sums), _stream_arg(stream))


def grid_corridor_device(sums, points, planes, x0: float, y0: float, cell: float, reach: int = 8, slot0: int = 0,
                         rect=None, status=None, stream=None):
    """sums (H + 1, W + 1) int32 from ``grid_occ_sums_device``, points (B, N, 3) fp64, planes (B, N, nobst, 4) fp64 whose
    slots slot0 .. slot0 + 3 are written, rect (B, N, 4) and status (B, N) int32 or None: one rectangle of free cells
    and its four faces per (robot, stage) (``rmpc_grid_corridor_device``)."""
    H, W = int(sums.shape[0]) - 1, int(sums.shape[1]) - 1
    B, N, nobst = int(points.shape[0]), int(points.shape[1]), int(planes.shape[2])
    if tuple(planes.shape) != (B, N, nobst, 4) or tuple(points.shape) != (B, N, 3) or \
            (rect is not None and tuple(rect.shape) != (B, N, 4)) or (status is not None and tuple(status.shape) != (B, N)):
        raise ValueError("grid_corridor_device: need points (B, N, 3), planes (B, N, nobst, 4), rect (B, N, 4), status (B, N)")
    _grid_call("rmpc_grid_corridor_device", H, W, _ptr(sums), float(x0), float(y0), float(cell), B, N, _ptr(points),
               int(reach), nobst, int(slot0), _ptr(planes), None if rect is None else _ptr(rect),
               None if status is None else _ptr(status), _stream_arg(stream))


# the limits of the traffic-aware routes (include/rmpc_traffic.h)
TRAFFIC_PLANES, TRAFFIC_MAX_EDGE, TRAFFIC_MAX_CAP_VISIT, TRAFFIC_MAX_CAP_CONTRA, TRAFFIC_INF = (
    _abi.traffic_constants["RMPC_TRAFFIC_" + n] for n in ("PLANES", "MAX_EDGE", "MAX_CAP_VISIT", "MAX_CAP_CONTRA", "INF"))


def traffic_costs(base_axial: int = 1000, base_diag: int = 1414, w_visit: int = 300, cap_visit: int = 32,
                  w_contra: int = 700, cap_contra: int = 15) -> TrafficCostsArgs:
    """The ``rmpc_traffic_costs`` of include/rmpc_traffic.h.  The defaults are the weights of the rule's numpy prototype,
    a documented starting point nobody has tuned, with caps that keep the largest edge cost
    1414 + 300 * 32 + 700 * 15 = 21514 below ``TRAFFIC_MAX_EDGE``."""
    c = TrafficCostsArgs()
    c.struct_size = C.sizeof(TrafficCostsArgs)
    c.base_axial, c.base_diag = int(base_axial), int(base_diag)
    c.w_visit, c.cap_visit, c.w_contra, c.cap_contra = int(w_visit), int(cap_visit), int(w_contra), int(cap_contra)
    return c


def _flow_check(name, flow, H, W):
    if tuple(flow.shape) != (TRAFFIC_PLANES, H, W) or flow.element_size() != 4 or not flow.is_contiguous():
        raise ValueError(name + ": need a contiguous int32 flow table (%d, H, W)" % TRAFFIC_PLANES)


def grid_traffic_add_device(flow, path, length, sign: int = 1, select=None, stream=None):
    """flow (9, H, W) int32, path (B, max_len) int32, length (B,) int32, select (B,) int32 or None: adds ``sign`` times
    the routes of the robots with length > 0 (and select != 0) to the flow table (``rmpc_grid_traffic_add_device``,
    include/rmpc_traffic.h)."""
    H, W = int(flow.shape[1]), int(flow.shape[2])
    _flow_check("grid_traffic_add_device", flow, H, W)
    B = int(path.shape[0])
    if tuple(length.shape) != (B,) or (select is not None and tuple(select.shape) != (B,)) or not path.is_contiguous():
        raise ValueError("grid_traffic_add_device: need a contiguous path (B, max_len), length (B,) and select (B,)")
    _grid_call("rmpc_grid_traffic_add_device", H, W, B, _ptr(path), _ptr(length), int(path.shape[1]),
               None if select is None else _ptr(select), int(sign), _ptr(flow), _stream_arg(stream))


def grid_fields_traffic_device(grid, flow, costs, goal_cells, fields, status, movement: int = 8, occ_threshold: float = 0.8,
                               sweeps=None, stream=None):
    """grid (H, W) fp64, flow (9, H, W) int32, costs a ``traffic_costs()``, goal_cells (G,) int32, fields (G, H, W) int32,
    status (G,) int32, sweeps (G,) int32 or None: one cost-to-go field per goal on the edge costs of the flow table
    (``rmpc_grid_fields_traffic_device``)."""
    H, W = int(grid.shape[0]), int(grid.shape[1])
    G = int(goal_cells.shape[0])
    _flow_check("grid_fields_traffic_device", flow, H, W)
    if tuple(fields.shape) != (G, H, W) or fields.element_size() != 4 or not fields.is_contiguous() or not grid.is_contiguous():
        raise ValueError("grid_fields_traffic_device: need a contiguous grid (H, W) and contiguous int32 fields (G, H, W)")
    _grid_call("rmpc_grid_fields_traffic_device", H, W, _ptr(grid), float(occ_threshold), _ptr(flow), C.byref(costs), G,
               _ptr(goal_cells), int(movement), _ptr(fields), _ptr(status), None if sweeps is None else _ptr(sweeps),
               _stream_arg(stream))


def grid_paths_traffic_device(grid, flow, costs, fields, goal_cells, start_cell, goal_index, path, length, movement: int = 8,
                              occ_threshold: float = 0.8, stream=None):
    """start_cell, goal_index (B,) int32, path (B, max_len) int32, length (B,) int32: descent of the traffic-aware
    fields (G, H, W) int32 on the table and costs they were made with (``rmpc_grid_paths_traffic_device``)."""
    H, W = int(grid.shape[0]), int(grid.shape[1])
    G, B = int(goal_cells.shape[0]), int(start_cell.shape[0])
    _flow_check("grid_paths_traffic_device", flow, H, W)
    if tuple(fields.shape)[1:] != (H, W) or int(fields.shape[0]) < G or fields.element_size() != 4 or \
            not fields.is_contiguous() or tuple(goal_index.shape) != (B,) or int(path.shape[0]) != B or \
            tuple(length.shape) != (B,) or not path.is_contiguous():
        raise ValueError("grid_paths_traffic_device: need int32 fields (G, H, W), start_cell, goal_index, length (B,) and "
                         "a contiguous path (B, max_len)")
    _grid_call("rmpc_grid_paths_traffic_device", H, W, _ptr(grid), float(occ_threshold), _ptr(flow), C.byref(costs), G,
               _ptr(fields), _ptr(goal_cells), B, _ptr(start_cell), _ptr(goal_index), int(movement), int(path.shape[1]),
               _ptr(path), _ptr(length), _stream_arg(stream))


def grid_traffic_score_device(flow, score, base_axial: int = 1000, base_diag: int = 1414, stream=None):
    """flow (9, H, W) int32 -> score (3,) int64: (L, V, C) of the table (``rmpc_grid_traffic_score_device``)."""
    H, W = int(flow.shape[1]), int(flow.shape[2])
    _flow_check("grid_traffic_score_device", flow, H, W)
    if tuple(score.shape) != (3,) or score.element_size() != 8 or not score.is_contiguous():
        raise ValueError("grid_traffic_score_device: need a contiguous int64 score (3,)")
    _grid_call("rmpc_grid_traffic_score_device", H, W, _ptr(flow), int(base_axial), int(base_diag), _ptr(score),
               _stream_arg(stream))


def lidar_args(pose, points, boxes=None, circles=None, angle_min: float = -np.pi, angle_max: float = np.pi,
               max_range: float = 10.0, offset=(0.4, 0.0), height: float = 0.02, ranges=None) -> LidarArgs:
    """The ``rmpc_lidar`` of one scan: pose (B, stride >= 3) fp64 (e.g. xinit), points (B, R, 3) fp64, boxes (nbox, 4)
    and circles (ncircle, 3) fp64 or None, ranges (B, R) fp64 or None -- contiguous device tensors."""
    a = LidarArgs()
    a.struct_size = C.sizeof(LidarArgs)
    a.rays = int(points.shape[1])
    a.angle_min, a.angle_max, a.range = float(angle_min), float(angle_max), float(max_range)
    a.offset_x, a.offset_y, a.height = float(offset[0]), float(offset[1]), float(height)
    a.pose, a.pose_stride = pose.data_ptr(), int(pose.stride(0))
    a.nbox = 0 if boxes is None else int(boxes.shape[0])
    a.boxes = None if boxes is None or a.nbox == 0 else boxes.data_ptr()
    a.ncircle = 0 if circles is None else int(circles.shape[0])
    a.circles = None if circles is None or a.ncircle == 0 else circles.data_ptr()
    a.points = points.data_ptr()
    a.ranges = None if ranges is None else ranges.data_ptr()
    return a


def lidar_scan_device(pose, points, boxes=None, circles=None, angle_min: float = -np.pi, angle_max: float = np.pi,
                      max_range: float = 10.0, offset=(0.4, 0.0), height: float = 0.02, ranges=None, stream=None):
    """One lidar scan of B robots (``rmpc_lidar_scan_device``): R = points.shape[1] rays per robot into the shared
    world of boxes (cx, cy, lx, ly) and circles (cx, cy, r); points (B, R, 3) = the absolute cloud of the reference's
    ``compute_point_cloud``, ranges (B, R) the hit distances (max_range on a miss)."""
    a = lidar_args(pose, points, boxes, circles, angle_min, angle_max, max_range, offset, height, ranges)
    _grid_call("rmpc_lidar_scan_device", int(points.shape[0]), C.byref(a), _stream_arg(stream))


# entries of k_lidar_fleet's LDS list (kFleetListMax, csrc/rmpc_sense.hpp): with more bodies in range it drains and refills
LIDAR_FLEET_LIST = 512


def lidar_bodies_args(centres, radius, self0: int = 0, owner=None, static_ranges=None) -> LidarBodiesArgs:
    """The ``rmpc_lidar_bodies`` of one fleet scan: centres (P, stride >= 2) or (P, 1, 3) fp64 (the output of
    ``fleet_points_device`` with N = 1), radius (P,) fp64; owner (B, R) int32 and static_ranges (B, R) fp64 or None --
    contiguous device tensors.  Scanning robot b is body self0 + b."""
    a = LidarBodiesArgs()
    a.struct_size = C.sizeof(LidarBodiesArgs)
    a.P = int(centres.shape[0])
    a.centres = centres.data_ptr() if a.P else None
    a.centre_stride = int(centres.stride(0)) if a.P else max(2, int(centres.shape[-1]))
    a.radius = radius.data_ptr() if a.P else None
    a.self0 = int(self0)
    a.owner = None if owner is None else owner.data_ptr()
    a.static_ranges = None if static_ranges is None else static_ranges.data_ptr()
    return a


def lidar_scan_fleet_device(pose, points, centres, radius, boxes=None, circles=None, angle_min: float = -np.pi,
                            angle_max: float = np.pi, max_range: float = 10.0, offset=(0.4, 0.0), height: float = 0.02,
                            self0: int = 0, owner=None, static_ranges=None, ranges=None, stream=None):
    """One lidar scan of B robots that also sees the fleet (``rmpc_lidar_scan_fleet_device``): the scan of
    ``lidar_scan_device`` plus one round body per (centres [j], radius [j]), the scanning robot's own body self0 + b
    left out.  owner (B, R) int32 = the body a ray ended on, -2 the static world, -1 nothing; static_ranges (B, R) =
    the hit distances of the static world alone."""
    a = lidar_args(pose, points, boxes, circles, angle_min, angle_max, max_range, offset, height, ranges)
    f = lidar_bodies_args(centres, radius, self0, owner, static_ranges)
    _grid_call("rmpc_lidar_scan_fleet_device", int(points.shape[0]), C.byref(a), C.byref(f), _stream_arg(stream))


def plan_points_device(pose, points, z_prev=None, exitflag=None, offset=(0.4, 0.0), height: float = 0.02, stream=None):
    """Seeds of the free-space decomposition (``rmpc_plan_points_device``): points (B, N, 3) = the sensor origin of
    stage k of the previous plan z_prev (B, N, nvar), or of the current pose (B, stride >= 3) when z_prev is None or
    exitflag (B,) int32 [b] < 0."""
    B, N = int(points.shape[0]), int(points.shape[1])
    nvar = 3 if z_prev is None else int(z_prev.shape[2])
    _grid_call("rmpc_plan_points_device", B, N, None if z_prev is None else _ptr(z_prev), nvar,
               None if exitflag is None else _ptr(exitflag), _ptr(pose), int(pose.stride(0)), float(offset[0]),
               float(offset[1]), float(height), _ptr(points), _stream_arg(stream))


def fleet_points_device(pose, points, z_prev=None, exitflag=None, heading: int = 1, offset=(0.4, 0.0),
                        height: float = 0.0, stream=None):
    """Predicted collision points of the coming solve (``rmpc_fleet_points_device``): points (B, N, 3) from stage
    min(k + 1, N - 1) of the previous plan z_prev (B, N, nvar), or from the current pose (B, stride >= 3) when z_prev is
    None or exitflag (B,) int32 [b] < 0; heading 1 = the boxer's end link at ``offset``, 0 = (q0, q1, height)."""
    B, N = int(points.shape[0]), int(points.shape[1])
    nvar = 3 if z_prev is None else int(z_prev.shape[2])
    _grid_call("rmpc_fleet_points_device", B, N, None if z_prev is None else _ptr(z_prev), nvar,
               None if exitflag is None else _ptr(exitflag), _ptr(pose), int(pose.stride(0)), int(heading),
               float(offset[0]), float(offset[1]), float(height), _ptr(points), _stream_arg(stream))


def fleet_planes_device(points, radius, planes, K: int, max_range: float = float("inf"), slot0: int = 0, stream=None):
    """Separating planes against the K nearest neighbours (``rmpc_fleet_planes_device``): points (B, N, 3), radius (B,)
    fp64, planes (B, N, nobst, 4) fp64 whose slots slot0 .. slot0 + K - 1 are written."""
    B, N, nobst = int(points.shape[0]), int(points.shape[1]), int(planes.shape[2])
    _grid_call("rmpc_fleet_planes_device", B, N, _ptr(points), _ptr(radius), int(K), float(max_range), nobst, int(slot0),
               _ptr(planes), _stream_arg(stream))


def grid_mark_args(origins, points, ranges, hits, misses, x0: float, y0: float, cell: float, max_range: float = 10.0,
                   hit_depth: float = 1e-6, skipped=None) -> GridMarkArgs:
    """The ``rmpc_grid_mark`` of one scan: origins (B, 1, 3) or (B, 3), points (B, R, 3), ranges (B, R) fp64; hits,
    misses (H, W) int32; skipped a one-element int32 tensor or None -- contiguous device tensors."""
    a = GridMarkArgs()
    a.struct_size = C.sizeof(GridMarkArgs)
    a.rays = int(points.shape[1])
    a.origins, a.points, a.ranges = origins.data_ptr(), points.data_ptr(), ranges.data_ptr()
    a.range, a.hit_depth = float(max_range), float(hit_depth)
    a.H, a.W = int(hits.shape[0]), int(hits.shape[1])
    a.x0, a.y0, a.cell = float(x0), float(y0), float(cell)
    a.hits, a.misses = hits.data_ptr(), misses.data_ptr()
    a.skipped = None if skipped is None else skipped.data_ptr()
    return a


def grid_mark_device(origins, points, ranges, hits, misses, x0: float, y0: float, cell: float, max_range: float = 10.0,
                     hit_depth: float = 1e-6, skipped=None, stream=None):
    """Adds one lidar scan of B robots to the evidence grids (``rmpc_grid_mark_device``): every ray origins [b] ->
    points [b][i] is walked cell by cell, misses += 1 on the cells it crosses, hits += 1 on the cell ``hit_depth``
    behind the end point of a ray that hit (ranges < max_range); skipped counts the rays left out."""
    a = grid_mark_args(origins, points, ranges, hits, misses, x0, y0, cell, max_range, hit_depth, skipped)
    _grid_call("rmpc_grid_mark_device", int(points.shape[0]), C.byref(a), _stream_arg(stream))


def grid_occupancy_device(hits, misses, grid, free_value: float, occ_value: float, unknown_value: float, w_hit: int = 3,
                          w_miss: int = 1, forget: int = 0, stream=None):
    """hits, misses (H, W) int32, grid (H, W) fp64: the class of every cell (``rmpc_grid_occupancy_device``) --
    unknown without evidence, occupied when hits w_hit > misses w_miss, free otherwise; forget > 0 then shifts both
    counters right by that many bits."""
    H, W = int(hits.shape[0]), int(hits.shape[1])
    _grid_call("rmpc_grid_occupancy_device", H, W, _ptr(hits), _ptr(misses), int(w_hit), int(w_miss), int(forget),
               float(free_value), float(occ_value), float(unknown_value), _ptr(grid), _stream_arg(stream))


def grid_frontier_device(hits, misses, enlarged, plan, seed, count, occ_threshold: float = 0.8, nmoves: int = 4,
                         unknown_value: float = 1.0, stream=None):
    """hits, misses (H, W) int32, enlarged (H, W) fp64 -> plan, seed (H, W) fp64 and count (1,) int32, which grows by
    the number of frontier cells (``rmpc_grid_frontier_device``): plan is ``enlarged`` on the cells with evidence and
    unknown_value elsewhere, seed 0 on the frontier (known, free on ``enlarged``, an unknown neighbour among the first
    nmoves moves) and +inf elsewhere."""
    H, W = int(hits.shape[0]), int(hits.shape[1])
    _grid_call("rmpc_grid_frontier_device", H, W, _ptr(hits), _ptr(misses), _ptr(enlarged), float(occ_threshold),
               int(nmoves), float(unknown_value), _ptr(plan), _ptr(seed), _ptr(count), _stream_arg(stream))


def grid_tiles(H: int, W: int, tile: int) -> int:
    """T = ceil(H / tile) ceil(W / tile), the tiles (and targets) of ``rmpc_grid_targets_device``."""
    if int(tile) < 1:
        raise ValueError("grid_tiles: need tile >= 1")
    return -(-int(H) // int(tile)) * -(-int(W) // int(tile))


def grid_targets_device(seed, tile: int, target_cells, tseeds=None, stream=None):
    """seed (H, W) fp64 (the seed of ``grid_frontier_device``) -> target_cells (T,) int32 and, when given, tseeds
    (T, H, W) fp64 with T = ``grid_tiles(H, W, tile)``: per tile of tile x tile cells the source nearest the centroid of
    the tile's sources, -1 without one; tseeds[t] is 0 at that cell and +inf elsewhere (``rmpc_grid_targets_device``)."""
    H, W = int(seed.shape[0]), int(seed.shape[1])
    T = grid_tiles(H, W, tile)
    if int(target_cells.shape[0]) != T or (tseeds is not None and tuple(tseeds.shape) != (T, H, W)):
        raise ValueError(f"grid_targets_device: {H}x{W} cells in tiles of {int(tile)} need target_cells ({T},) and "
                         f"tseeds ({T}, {H}, {W})")
    _grid_call("rmpc_grid_targets_device", H, W, _ptr(seed), int(tile), _ptr(target_cells),
               None if tseeds is None else _ptr(tseeds), _stream_arg(stream))


def grid_route_costs_device(grid, fields, start_cell, cost, movement: int = 8, occ_threshold: float = 0.8,
                            cost_factor: float = 3.0, stream=None):
    """grid (H, W) fp64, fields (T, H, W) fp64, start_cell (B,) int32 -> cost (B, T) fp64: the field's value at the
    robot's cell, from an occupied cell the best step out of it, +inf outside the map
    (``rmpc_grid_route_costs_device``)."""
    H, W = int(grid.shape[0]), int(grid.shape[1])
    B, T = int(start_cell.shape[0]), int(fields.shape[0])
    if tuple(fields.shape) != (T, H, W) or tuple(cost.shape) != (B, T):
        raise ValueError(f"grid_route_costs_device: need fields ({T}, {H}, {W}) and cost ({B}, {T})")
    _grid_call("rmpc_grid_route_costs_device", H, W, _ptr(grid), T, _ptr(fields), B, _ptr(start_cell), int(movement),
               float(occ_threshold), float(cost_factor), _ptr(cost), _stream_arg(stream))


def assign_greedy_device(cost, assign, passes=None, stream=None):
    """cost (B, T) fp64 -> assign (B,) int32, the target of every robot or -1, and passes (B,) int32 or None, the pass
    (from 0) in which it was taken or -1: greedy assignment by (cost, b, t) in passes (``rmpc_assign_greedy_device``)."""
    B, T = int(cost.shape[0]), int(cost.shape[1])
    if int(assign.shape[0]) != B or (passes is not None and int(passes.shape[0]) != B):
        raise ValueError(f"assign_greedy_device: need assign and passes ({B},)")
    _grid_call("rmpc_assign_greedy_device", B, T, _ptr(cost), _ptr(assign), None if passes is None else _ptr(passes),
               _stream_arg(stream))


# the greatest integer cost of a takeable pair (include/rmpc_assign_opt.h)
ASSIGN_OPT_MAX_Q = _abi.assign_constants["RMPC_ASSIGN_OPT_MAX_Q"]


def assign_optimal_work_bytes(G: int, B: int, T: int) -> int:
    """The bytes of workspace ``assign_optimal_device`` needs for G problems of B x T
    (``rmpc_assign_optimal_work_bytes``; host only)."""
    return _size_query("rmpc_assign_optimal_work_bytes", G, B, T)


def assign_optimal_device(cost, assign, scale: float = 1024.0, total=None, count=None, steps=None, work=None, stream=None):
    """cost (B, T) or (G, B, T) fp64 -> assign (B,) or (G, B) int32, the target of every robot or -1: per problem the
    matching with the most takeable pairs and among those the least sum of q = rint(cost scale), by shortest augmenting
    paths on integers (``rmpc_assign_optimal_device``).  total (G,) int64, count (G,) int32, steps (G,) int32 or None:
    the sum of q, the number of pairs, the steps of the search.  work: a contiguous device tensor of at least
    ``assign_optimal_work_bytes(G, B, T)`` bytes, allocated here when None."""
    import torch
    if cost.dim() not in (2, 3) or cost.dtype != torch.float64 or not cost.is_contiguous():
        raise ValueError("assign_optimal_device: need cost (B, T) or (G, B, T), contiguous fp64")
    G = 1 if cost.dim() == 2 else int(cost.shape[0])
    B, T = int(cost.shape[-2]), int(cost.shape[-1])
    if tuple(assign.shape) != tuple(cost.shape[:-1]) or assign.dtype != torch.int32 or not assign.is_contiguous():
        raise ValueError(f"assign_optimal_device: need assign {tuple(cost.shape[:-1])} contiguous int32")
    for name, t, dt in (("total", total, torch.int64), ("count", count, torch.int32), ("steps", steps, torch.int32)):
        if t is not None and (t.numel() != G or t.dtype != dt or not t.is_contiguous()):
            raise ValueError(f"assign_optimal_device: need {name} ({G},) contiguous {dt}")
    need = assign_optimal_work_bytes(G, B, T)
    if work is None:
        work = torch.empty(need, dtype=torch.uint8, device=cost.device)
    if not work.is_contiguous():
        raise ValueError("assign_optimal_device: need a contiguous workspace")
    opt = lambda t: None if t is None else _ptr(t)
    _grid_call("rmpc_assign_optimal_device", G, B, T, _ptr(cost), float(scale), _ptr(assign), opt(total), opt(count),
               opt(steps), _ptr(work), int(work.numel() * work.element_size()), _stream_arg(stream))


# limits of the tours (include/rmpc_tours.h)
TOURS_MAX_ROBOTS, TOURS_MAX_TASKS = (_abi.tours_constants["RMPC_TOURS_MAX_" + n] for n in ("ROBOTS", "TASKS"))
TOURS_MODES = {"sum": 0, "span": 1, 0: 0, 1: 1}


def tours_work_bytes(G: int, B: int, T: int) -> int:
    """The bytes of workspace ``tours_device`` needs for G problems of B robots and T tasks (``rmpc_tours_work_bytes``;
    host only)."""
    return _size_query("rmpc_tours_work_bytes", G, B, T)


def tours_device(start_cost, task_cost, tours, lens, cost, mode="span", scale: float = 1024.0, max_rounds: int = 1 << 30,
                 owner=None, count=None, total=None, span=None, build_steps=None, rounds=None, work=None, stream=None):
    """start_cost (B, T) or (G, B, T), task_cost (T, T) or (G, T, T) fp64 -> tours (.., B, K) int32 (every robot's tasks
    in order, padded with -1), lens (.., B) int32, cost (.., B) int64: cheapest insertion, then the best relocation or
    exchange per round, at most ``max_rounds`` of them, on q = rint(cost scale) (``rmpc_tours_device``,
    include/rmpc_tours.h).  mode "sum" (0) or "span" (1).  owner (.., T) int32, count (G,) int32, total, span (G,) int64,
    build_steps, rounds (G,) int32, or None.  work: a contiguous device tensor of at least ``tours_work_bytes(G, B, T)``
    bytes, allocated here when None."""
    import torch
    if start_cost.dim() not in (2, 3) or task_cost.dim() != start_cost.dim() or tours.dim() != start_cost.dim():
        raise ValueError("tours_device: need start_cost (B, T) or (G, B, T), task_cost and tours of as many dimensions")
    G = 1 if start_cost.dim() == 2 else int(start_cost.shape[0])
    lead = tuple(start_cost.shape[:-2])
    B, T, K = int(start_cost.shape[-2]), int(start_cost.shape[-1]), int(tours.shape[-1])
    if mode not in TOURS_MODES:
        raise ValueError("tours_device: mode must be 'sum' or 'span'")
    for name, t, shape, dt in (("start_cost", start_cost, lead + (B, T), torch.float64),
                               ("task_cost", task_cost, lead + (T, T), torch.float64),
                               ("tours", tours, lead + (B, K), torch.int32), ("lens", lens, lead + (B,), torch.int32),
                               ("cost", cost, lead + (B,), torch.int64), ("owner", owner, lead + (T,), torch.int32)):
        if t is not None and (tuple(t.shape) != shape or t.dtype != dt or not t.is_contiguous()):
            raise ValueError(f"tours_device: need {name} {shape} contiguous {dt}")
    for name, t, dt in (("count", count, torch.int32), ("total", total, torch.int64), ("span", span, torch.int64),
                        ("build_steps", build_steps, torch.int32), ("rounds", rounds, torch.int32)):
        if t is not None and (t.numel() != G or t.dtype != dt or not t.is_contiguous()):
            raise ValueError(f"tours_device: need {name} ({G},) contiguous {dt}")
    need = tours_work_bytes(G, B, T)
    if work is None:
        work = torch.empty(need, dtype=torch.uint8, device=start_cost.device)
    if not work.is_contiguous():
        raise ValueError("tours_device: need a contiguous workspace")
    opt = lambda t: None if t is None else _ptr(t)
    _grid_call("rmpc_tours_device", G, B, T, K, _ptr(start_cost), _ptr(task_cost), TOURS_MODES[mode], float(scale),
               int(max_rounds), _ptr(tours), _ptr(lens), _ptr(cost), opt(owner), opt(count), opt(total), opt(span),
               opt(build_steps), opt(rounds), _ptr(work), int(work.numel() * work.element_size()), _stream_arg(stream))


def follow_tour_device(path, length, idx, pos, goal, W: int, x0: float, y0: float, cell: float, threshold: float,
                       stop_at, leg, served, now: int, stop_tol: float, stream=None):
    """``follow_path_device`` with stops: stop_at (B, K) int32 ascending path indices (-1 unused), leg (B,) int32 the
    stops served (in and out), served (B, K) int32 takes ``now`` where a stop is served (``rmpc_follow_tour_device``)."""
    _grid_call("rmpc_follow_tour_device", int(path.shape[0]), _ptr(path), _ptr(length), int(path.shape[1]), _ptr(idx),
               _ptr(pos), int(pos.stride(0)), int(W), float(x0), float(y0), float(cell), float(threshold), _ptr(goal),
               int(stop_at.shape[1]), _ptr(stop_at), _ptr(leg), _ptr(served), int(now), float(stop_tol),
               _stream_arg(stream))


def grid_edge_distance_device(grid, d2, occ_threshold: float, sub: int, cap: int, stream=None):
    """grid (H, W) fp64 -> d2 (H sub, W sub) int32: per fine cell the squared distance, in fine cells and capped at
    ``cap``, to the nearest fine cell of the other class (``rmpc_grid_edge_distance_device``)."""
    H, W = int(grid.shape[0]), int(grid.shape[1])
    if tuple(d2.shape) != (H * int(sub), W * int(sub)):
        raise ValueError(f"grid_edge_distance_device: need d2 ({H * int(sub)}, {W * int(sub)})")
    _grid_call("rmpc_grid_edge_distance_device", H, W, _ptr(grid), float(occ_threshold), int(sub), int(cap), _ptr(d2),
               _stream_arg(stream))


def lidar_project_device(pose, ranges, points, angle_min: float = -np.pi, angle_max: float = np.pi,
                         max_range: float = 10.0, offset=(0.4, 0.0), height: float = 0.02, stream=None):
    """The ranges (B, R) of a scan as points (B, R, 3) at the believed pose (B, stride >= 3), formed as the scan forms
    them (``rmpc_lidar_project_device``)."""
    a = lidar_args(pose, points, None, None, angle_min, angle_max, max_range, offset, height, ranges)
    _grid_call("rmpc_lidar_project_device", int(points.shape[0]), C.byref(a), _stream_arg(stream))


def scan_match_args(pose, points, ranges, d2, rot, pose_out, best, score, H: int, W: int, sub: int, cap: int, x0: float,
                    y0: float, cell: float, nxy: int, step_xy: float, nth: int, step_th: float, max_range: float = 10.0,
                    min_hits: int = 8, score0=None, used=None) -> ScanMatchArgs:
    """The ``rmpc_scan_match`` of one scan: pose (B, stride >= 3), points (B, R, 3), ranges (B, R) fp64; d2
    (H sub, W sub) int32; rot (2 nth + 1, 2) fp64; pose_out (B, 3) fp64; best, score and, when given, score0, used (B,)
    int32 -- contiguous device tensors."""
    a = ScanMatchArgs()
    a.struct_size = C.sizeof(ScanMatchArgs)
    a.rays = int(points.shape[1])
    a.pose, a.points, a.ranges = pose.data_ptr(), points.data_ptr(), ranges.data_ptr()
    a.range, a.pose_stride, a.min_hits = float(max_range), int(pose.stride(0)), int(min_hits)
    a.d2, a.H, a.W, a.sub, a.cap = d2.data_ptr(), int(H), int(W), int(sub), int(cap)
    a.x0, a.y0, a.cell = float(x0), float(y0), float(cell)
    a.nxy, a.nth, a.step_xy, a.step_th = int(nxy), int(nth), float(step_xy), float(step_th)
    a.rot = rot.data_ptr()
    a.pose_out, a.best, a.score = pose_out.data_ptr(), best.data_ptr(), score.data_ptr()
    a.score0 = None if score0 is None else score0.data_ptr()
    a.used = None if used is None else used.data_ptr()
    return a


def scan_match_device(args: ScanMatchArgs, B: int, stream=None):
    """Correlative scan matching of B robots (``rmpc_scan_match_device``) with the ``scan_match_args`` of the call."""
    _grid_call("rmpc_scan_match_device", int(B), C.byref(args), _stream_arg(stream))


# limits of the wide-window search: nxy, nth (include/rmpc.h), top_log2 and the pyramid's levels (kSearchMaxTop,
# kSearchMaxLevels, csrc/rmpc_search.hpp)
SEARCH_MAX_N, = _k("SEARCH_MAX_N")
SEARCH_MAX_TOP, SEARCH_MAX_LEVELS = 7, 12


def grid_min_pyramid_device(d2, pyr, sub: int, stream=None):
    """d2 (H sub, W sub) int32 -> pyr (levels, H sub, W sub) int32: per level l and fine cell the least d2 over the
    window of side 2^l that starts there, cut at the map's edge (``rmpc_grid_min_pyramid_device``)."""
    FH, FW, sub = int(d2.shape[0]), int(d2.shape[1]), int(sub)
    if sub < 1 or FH % sub or FW % sub or pyr.dim() != 3 or tuple(pyr.shape[1:]) != (FH, FW):
        raise ValueError(f"grid_min_pyramid_device: need d2 (H sub, W sub) and pyr (levels, {FH}, {FW})")
    _grid_call("rmpc_grid_min_pyramid_device", FH // sub, FW // sub, sub, _ptr(d2), int(pyr.shape[0]), _ptr(pyr),
               _stream_arg(stream))


def scan_search_top_nodes(nxy: int, nth: int, top_log2: int) -> int:
    """the top-level nodes of one robot: (2 nth + 1) nb nb, nb = ceil((2 nxy + 1) / 2^top_log2)"""
    nb = -(-(2 * int(nxy) + 1) // (1 << int(top_log2)))
    return (2 * int(nth) + 1) * nb * nb


def scan_search_work_bytes(B: int, nxy: int, nth: int, top_log2: int) -> int:
    """bytes of workspace of ``scan_search_device`` (``rmpc_scan_search_work_bytes``)"""
    return _size_query("rmpc_scan_search_work_bytes", B, nxy, nth, top_log2)


def scan_search_args(match: ScanMatchArgs, pyr, top_log2: int, work, active=None, leaves=None,
                     top_bound=None) -> ScanSearchArgs:
    """The ``rmpc_scan_search`` of one scan: the ``scan_match_args`` of the call (nxy, nth up to ``SEARCH_MAX_N``), pyr
    (levels, H sub, W sub) int32, work a uint8 tensor of ``scan_search_work_bytes``, and, when given, active, leaves (B,)
    and top_bound (B, ``scan_search_top_nodes``) int32 -- contiguous device tensors."""
    a = ScanSearchArgs()
    for name, _ in ScanMatchArgs._fields_:
        setattr(a, name, getattr(match, name))
    a.struct_size = C.sizeof(ScanSearchArgs)
    a.pyr, a.levels, a.top_log2 = pyr.data_ptr(), int(pyr.shape[0]), int(top_log2)
    a.active = None if active is None else active.data_ptr()
    a.work, a.work_bytes = work.data_ptr(), int(work.numel()) * int(work.element_size())
    a.leaves = None if leaves is None else leaves.data_ptr()
    a.top_bound = None if top_bound is None else top_bound.data_ptr()
    return a


def scan_search_device(args: ScanSearchArgs, B: int, stream=None):
    """Branch-and-bound scan matching of B robots (``rmpc_scan_search_device``) with the ``scan_search_args`` of the
    call."""
    _grid_call("rmpc_scan_search_device", int(B), C.byref(args), _stream_arg(stream))


# limits of the moving-obstacle tracker (include/rmpc.h)
TRACK_MAX_RAYS, TRACK_MAX_TRACKS, TRACK_MAX_DET = _k("TRACK_MAX_RAYS", "TRACK_MAX_TRACKS", "TRACK_MAX_DET")


def tracks_args(points, ranges, origin, track, age, miss, obst_dyn, radius: float, dt: float, static_ranges=None,
                closed: bool = True, max_range: float = 10.0, margin: float = 0.05, gap: float = 0.3, min_rays: int = 2,
                max_extent: float = 0.0, gate: float = 1.0, alpha: float = 0.4, beta: float = 0.1, v_max: float = 0.0,
                confirm: int = 3, max_miss: int = 5, park=(100.0, 100.0), det=None, counts=None) -> TracksArgs:
    """The ``rmpc_tracks`` of one call: points (B, R, 3), ranges (B, R), origin (B, 3), track (B, T, 4), obst_dyn
    (B, n_out, 9) fp64; age, miss (B, T) int32; static_ranges (B, R) fp64, det (B, 16, 2) fp64 and counts (B, 4) int32 or
    None -- contiguous device tensors."""
    a = TracksArgs()
    a.struct_size = C.sizeof(TracksArgs)
    a.rays, a.closed, a.min_rays = int(points.shape[1]), int(bool(closed)), int(min_rays)
    a.points, a.ranges, a.origin = points.data_ptr(), ranges.data_ptr(), origin.data_ptr()
    a.static_ranges = None if static_ranges is None else static_ranges.data_ptr()
    a.range, a.margin, a.gap, a.radius, a.max_extent = float(max_range), float(margin), float(gap), float(radius), float(max_extent)
    a.gate, a.dt, a.alpha, a.beta, a.v_max = float(gate), float(dt), float(alpha), float(beta), float(v_max)
    a.park_x, a.park_y = float(park[0]), float(park[1])
    a.confirm, a.max_miss, a.n_tracks, a.n_out = int(confirm), int(max_miss), int(track.shape[1]), int(obst_dyn.shape[1])
    a.track, a.age, a.miss, a.obst_dyn = track.data_ptr(), age.data_ptr(), miss.data_ptr(), obst_dyn.data_ptr()
    a.det = None if det is None else det.data_ptr()
    a.counts = None if counts is None else counts.data_ptr()
    a._keep = (points, ranges, origin, static_ranges, track, age, miss, obst_dyn, det, counts)
    return a


def lidar_tracks_device(args: TracksArgs, B: int, stream=None):
    """One step of the moving-obstacle tracker of B robots (``rmpc_lidar_tracks_device``) with the ``tracks_args`` of
    the call: the filter's state (track, age, miss) is updated in place and obst_dyn written."""
    _grid_call("rmpc_lidar_tracks_device", int(B), C.byref(args), _stream_arg(stream))


# limits and the status of the timed routes (include/rmpc.h)
TIMED_MAX_ROBOTS, TIMED_MAX_T, TIMED_MAX_ORDERS, TIMED_MAX_SEP2, TIMED_MAX_LAG, TIMED_BAD_ORDER = _k(
    "TIMED_MAX_ROBOTS", "TIMED_MAX_T", "TIMED_MAX_ORDERS", "TIMED_MAX_SEP2", "TIMED_MAX_LAG", "TIMED_BAD_ORDER")


def timed_plan_work_bytes(H: int, W: int, T: int, G: int) -> int:
    """bytes of workspace of ``timed_plan_device`` (``rmpc_timed_plan_work_bytes``)"""
    return _size_query("rmpc_timed_plan_work_bytes", H, W, T, G)


def _timed_common(cls, grid, start_cell, fields, goal_cells, orders, work, paths, status, arrive, key, best, movement,
                  occ_threshold, sep2, lag):
    """a ``cls`` with what rmpc_timed_plan, rmpc_timed_tours and rmpc_timed_repair have in common filled in"""
    a = cls()
    a.struct_size = C.sizeof(cls)
    a.H, a.W, a.movement = int(grid.shape[0]), int(grid.shape[1]), int(movement)
    a.grid, a.occ_threshold = grid.data_ptr(), float(occ_threshold)
    a.B, a.Gf = int(start_cell.shape[0]), int(fields.shape[0])
    a.start_cell, a.fields, a.goal_cells = start_cell.data_ptr(), fields.data_ptr(), goal_cells.data_ptr()
    a.T, a.sep2, a.lag, a.G = int(paths.shape[2]) - 1, int(sep2), int(lag), int(orders.shape[0])
    a.orders = orders.data_ptr()
    a.work, a.work_bytes = work.data_ptr(), int(work.numel() * work.element_size())
    a.paths, a.status, a.arrive, a.key, a.best = (paths.data_ptr(), status.data_ptr(), arrive.data_ptr(), key.data_ptr(),
                                                  best.data_ptr())
    return a


def timed_plan_args(grid, start_cell, goal_index, fields, goal_cells, orders, work, paths, status, arrive, key, best,
                    movement: int = 4, occ_threshold: float = 0.8, sep2: int = 9, lag: int = 1) -> TimedPlanArgs:
    """The ``rmpc_timed_plan`` of one plan: grid (H, W) fp64, start_cell, goal_index (B,) int32, fields (Gf, H, W) fp64,
    goal_cells (Gf,) int32, orders (G, B) int32, work a uint8 tensor of ``timed_plan_work_bytes``, paths (G, B, T + 1),
    status, arrive (G, B) int32, key (G,) int64, best (1,) int32 -- contiguous device tensors."""
    a = _timed_common(TimedPlanArgs, grid, start_cell, fields, goal_cells, orders, work, paths, status, arrive, key, best,
                      movement, occ_threshold, sep2, lag)
    a.goal_index = goal_index.data_ptr()
    a._keep = (grid, start_cell, goal_index, fields, goal_cells, orders, work, paths, status, arrive, key, best)
    return a


def timed_plan_device(args: TimedPlanArgs, stream=None):
    """One prioritised space-time plan per order (``rmpc_timed_plan_device``)."""
    _grid_call("rmpc_timed_plan_device", C.byref(args), _stream_arg(stream))


def timed_follow_device(paths, idx_in, idx_out, pos, goal, W: int, x0: float, y0: float, cell: float, threshold: float,
                        sep2: int, lag: int = 1, blocked=None, stream=None):
    """paths (B, T + 1), idx_in, idx_out (B,) int32 (two buffers); pos (B, stride >= 2) fp64; goal (B, 3) fp64; blocked
    (B,) int32 or None: one simultaneous step of the order-preserving follower (``rmpc_timed_follow_device``)."""
    _grid_call("rmpc_timed_follow_device", int(paths.shape[0]), int(paths.shape[1]) - 1, _ptr(paths), _ptr(idx_in),
               _ptr(idx_out), _ptr(pos), int(pos.stride(0)), int(W), float(x0), float(y0), float(cell), float(threshold),
               int(sep2), int(lag), _ptr(goal), None if blocked is None else _ptr(blocked), _stream_arg(stream))


# limits of the timed tours (include/rmpc_timed_tours.h)
TIMED_TOURS_MAX_STOPS, TIMED_TOURS_MAX_DWELL = (_abi.timed_tours_constants["RMPC_TIMED_TOURS_MAX_" + n]
                                                for n in ("STOPS", "DWELL"))


def timed_tours_work_bytes(H: int, W: int, T: int, G: int) -> int:
    """bytes of workspace of ``timed_tours_plan_device`` (``rmpc_timed_tours_work_bytes``)"""
    return _size_query("rmpc_timed_tours_work_bytes", H, W, T, G)


def timed_tours_args(grid, start_cell, stops, lens, park_index, fields, goal_cells, orders, work, paths, status, arrive, key,
                     best, serve_at, served, unserved, dwell: int = 0, movement: int = 4, occ_threshold: float = 0.8,
                     sep2: int = 9, lag: int = 1) -> TimedToursArgs:
    """The ``rmpc_timed_tours`` of one plan: ``timed_plan_args`` with stops (B, K), lens, park_index (B,) int32 in place
    of goal_index, and the outputs serve_at (G, B, K), served (G, B), unserved (G,) int32 -- contiguous device tensors."""
    a = _timed_common(TimedToursArgs, grid, start_cell, fields, goal_cells, orders, work, paths, status, arrive, key, best,
                      movement, occ_threshold, sep2, lag)
    a.K, a.dwell = int(stops.shape[1]), int(dwell)
    a.stops, a.len, a.park_index = stops.data_ptr(), lens.data_ptr(), park_index.data_ptr()
    a.serve_at, a.served, a.unserved = serve_at.data_ptr(), served.data_ptr(), unserved.data_ptr()
    a._keep = (grid, start_cell, stops, lens, park_index, fields, goal_cells, orders, work, paths, status, arrive, key, best,
               serve_at, served, unserved)
    return a


def timed_tours_plan_device(args: TimedToursArgs, stream=None):
    """One prioritised space-time plan through every robot's stops per order (``rmpc_timed_tours_plan_device``)."""
    _grid_call("rmpc_timed_tours_plan_device", C.byref(args), _stream_arg(stream))


def timed_tours_follow_device(paths, idx_in, idx_out, pos, goal, W: int, x0: float, y0: float, cell: float, threshold: float,
                              sep2: int, lag: int, serve_at, leg, served, now: int, stop_tol: float, blocked=None,
                              stream=None):
    """``timed_follow_device`` with stops: serve_at (B, K) int32 (one order's), leg (B,) int32 in and out, served (B, K)
    int32; one simultaneous step of the follower that serves a stop only within ``stop_tol`` of it
    (``rmpc_timed_tours_follow_device``)."""
    _grid_call("rmpc_timed_tours_follow_device", int(paths.shape[0]), int(paths.shape[1]) - 1, _ptr(paths), _ptr(idx_in),
               _ptr(idx_out), _ptr(pos), int(pos.stride(0)), int(W), float(x0), float(y0), float(cell), float(threshold),
               int(sep2), int(lag), _ptr(goal), None if blocked is None else _ptr(blocked), int(serve_at.shape[1]),
               _ptr(serve_at), _ptr(leg), _ptr(served), int(now), float(stop_tol), _stream_arg(stream))


# limits and the status of the lifelong timed tours (include/rmpc_timed_replan.h)
TIMED_RESERVE_MAX_PATHS, TIMED_KEPT = (_abi.timed_replan_constants["RMPC_TIMED_" + n] for n in ("RESERVE_MAX_PATHS", "KEPT"))


def timed_reserve_words(H: int, W: int, T: int) -> int:
    """the 64-bit words of a reservation table: T + 1 layers of H ceil(W / 64) (``rmpc_timed_reserve_words``)"""
    return _size_query("rmpc_timed_reserve_words", H, W, T)


def timed_reserve_device(cells, res, H: int, W: int, sep2: int, lag: int = 1, use=None, clear: bool = True, stream=None):
    """cells (P, T + 1) int32, use (P,) int32 or None, res an int64 tensor of ``timed_reserve_words(H, W, T)`` words --
    contiguous device tensors: the discs of the cells on the map stamped into the table, after emptying it when
    ``clear`` (``rmpc_timed_reserve_device``)."""
    T = int(cells.shape[1]) - 1
    if res.element_size() != 8 or res.numel() < timed_reserve_words(H, W, T):
        raise ValueError("timed_reserve_device: need res of timed_reserve_words(H, W, T) 64-bit words")
    _grid_call("rmpc_timed_reserve_device", int(H), int(W), T, int(cells.shape[0]), _ptr(cells),
               None if use is None else _ptr(use), int(sep2), int(lag), int(bool(clear)), _ptr(res), _stream_arg(stream))


def timed_replan_work_bytes(H: int, W: int, T: int, G: int) -> int:
    """bytes of workspace of ``timed_tours_replan_device`` (``rmpc_timed_replan_work_bytes``)"""
    return _size_query("rmpc_timed_replan_work_bytes", H, W, T, G)


def timed_replan_args(work, res0=None, active=None, begin=None, clash=None) -> TimedReplanArgs:
    """The ``rmpc_timed_replan`` of one re-plan: work a uint8 tensor of ``timed_replan_work_bytes``, res0 the reservation
    table (64-bit words) or None, active, begin, clash (B,) int32 or None -- contiguous device tensors."""
    a = TimedReplanArgs()
    a.struct_size = C.sizeof(TimedReplanArgs)
    opt = lambda t: None if t is None else t.data_ptr()
    a.res0, a.active, a.begin, a.clash = opt(res0), opt(active), opt(begin), opt(clash)
    a.work, a.work_bytes = work.data_ptr(), int(work.numel() * work.element_size())
    a._keep = (work, res0, active, begin, clash)
    return a


def timed_tours_replan_device(args: TimedToursArgs, replan: TimedReplanArgs, stream=None):
    """``timed_tours_plan_device`` inside the layer frame of a plan under way: around the reserved routes, for the
    active robots, each from its begin layer (``rmpc_timed_tours_replan_device``).  ``args.work`` is not read."""
    _grid_call("rmpc_timed_tours_replan_device", C.byref(args), C.byref(replan), _stream_arg(stream))


# the limit of the timed routes with repaired orders (include/rmpc_timed_repair.h)
TIMED_MAX_ROUNDS = _abi.timed_repair_constants["RMPC_TIMED_MAX_ROUNDS"]


def timed_plan_repair_work_bytes(H: int, W: int, T: int, G: int, B: int) -> int:
    """bytes of workspace of ``timed_plan_repair_device`` (``rmpc_timed_plan_repair_work_bytes``)"""
    return _size_query("rmpc_timed_plan_repair_work_bytes", H, W, T, G, B)


def timed_repair_args(grid, start_cell, goal_index, fields, goal_cells, orders, work, paths, status, arrive, key, best,
                      order_out, rounds_run, round_best, rounds: int, movement: int = 4, occ_threshold: float = 0.8,
                      sep2: int = 9, lag: int = 1) -> TimedRepairArgs:
    """The ``rmpc_timed_repair`` of one plan: ``timed_plan_args`` with work a uint8 tensor of
    ``timed_plan_repair_work_bytes``, the number of repair rounds, and the outputs order_out (G, B), rounds_run,
    round_best (G,) int32 -- contiguous device tensors."""
    a = _timed_common(TimedRepairArgs, grid, start_cell, fields, goal_cells, orders, work, paths, status, arrive, key, best,
                      movement, occ_threshold, sep2, lag)
    a.goal_index = goal_index.data_ptr()
    a.rounds = int(rounds)
    a.order_out, a.rounds_run, a.round_best = order_out.data_ptr(), rounds_run.data_ptr(), round_best.data_ptr()
    a._keep = (grid, start_cell, goal_index, fields, goal_cells, orders, work, paths, status, arrive, key, best, order_out,
               rounds_run, round_best)
    return a


def timed_plan_repair_device(args: TimedRepairArgs, stream=None):
    """``timed_plan_device`` round after round per order: the robots that failed or came late are planned first in the
    next round, and every row reports its best round (``rmpc_timed_plan_repair_device``)."""
    _grid_call("rmpc_timed_plan_repair_device", C.byref(args), _stream_arg(stream))


# limits, outcomes and the places of info of the conflict-based search (include/rmpc_cbs.h)
CBS_MAX_ROBOTS, CBS_MAX_NODES, CBS_MAX_EXPAND, CBS_MAX_ROUNDS, CBS_INF, CBS_INFO = (
    _abi.cbs_constants["RMPC_CBS_" + n] for n in ("MAX_ROBOTS", "MAX_NODES", "MAX_EXPAND", "MAX_ROUNDS", "INF", "INFO"))
CBS_SOLVED, CBS_INFEASIBLE, CBS_POOL, CBS_ROUNDS, CBS_BAD_STATE = (
    _abi.cbs_constants["RMPC_CBS_" + n] for n in ("SOLVED", "INFEASIBLE", "POOL", "ROUNDS", "BAD_STATE"))
CBS_INFO_NAMES = ("OUTCOME", "NODE", "CONFLICT_FREE", "COST", "BOUND", "CREATED", "EXPANDED", "ROUNDS_RUN")
CBS_OUTCOME, CBS_NODE, CBS_CONFLICT_FREE, CBS_COST, CBS_BOUND, CBS_CREATED, CBS_EXPANDED, CBS_ROUNDS_RUN = (
    _abi.cbs_constants["RMPC_CBS_" + n] for n in CBS_INFO_NAMES)


def cbs_work_bytes(H: int, W: int, T: int, B: int, nodes: int, expand: int) -> int:
    """bytes of workspace of ``cbs_device`` (``rmpc_cbs_work_bytes``)"""
    return _size_query("rmpc_cbs_work_bytes", H, W, T, B, nodes, expand)


def cbs_args(grid, start_cell, goal_index, fields, goal_cells, work, paths, status, arrive, info, nodes: int, expand: int,
             rounds: int, resume: bool = False, movement: int = 4, occ_threshold: float = 0.8, sep2: int = 9,
             lag: int = 1) -> CbsArgs:
    """The ``rmpc_cbs`` of one call: grid (H, W) fp64, start_cell, goal_index (B,) int32, fields (Gf, H, W) fp64,
    goal_cells (Gf,) int32, work a uint8 tensor of ``cbs_work_bytes``, paths (B, T + 1), status, arrive (B,) and info
    (CBS_INFO,) int32 -- contiguous device tensors."""
    a = CbsArgs()
    a.struct_size = C.sizeof(CbsArgs)
    a.H, a.W, a.movement = int(grid.shape[0]), int(grid.shape[1]), int(movement)
    a.grid, a.occ_threshold = grid.data_ptr(), float(occ_threshold)
    a.B, a.Gf = int(start_cell.shape[0]), int(fields.shape[0])
    a.start_cell, a.goal_index = start_cell.data_ptr(), goal_index.data_ptr()
    a.fields, a.goal_cells = fields.data_ptr(), goal_cells.data_ptr()
    a.T, a.sep2, a.lag = int(paths.shape[1]) - 1, int(sep2), int(lag)
    a.nodes, a.expand, a.rounds, a.resume = int(nodes), int(expand), int(rounds), int(bool(resume))
    a.work, a.work_bytes = work.data_ptr(), int(work.numel() * work.element_size())
    a.paths, a.status, a.arrive, a.info = paths.data_ptr(), status.data_ptr(), arrive.data_ptr(), info.data_ptr()
    a._keep = (grid, start_cell, goal_index, fields, goal_cells, work, paths, status, arrive, info)
    return a


def cbs_device(args: CbsArgs, stream=None):
    """``args.rounds`` rounds of conflict-based search over the timed routes, from the root or, with ``args.resume``,
    from the state the workspace holds (``rmpc_cbs_device``)."""
    _grid_call("rmpc_cbs_device", C.byref(args), _stream_arg(stream))


# the focal conflict-based search (include/rmpc_ecbs.h): limits and outcomes are the conflict-based search's
ECBS_MAX_W_DEN, ECBS_MAX_W, ECBS_INFO, ECBS_LB, ECBS_NCONF = (
    _abi.ecbs_constants["RMPC_ECBS_" + n] for n in ("MAX_W_DEN", "MAX_W", "INFO", "LB", "NCONF"))
ECBS_INFO_NAMES = CBS_INFO_NAMES + ("LB", "NCONF")


def ecbs_work_bytes(H: int, W: int, T: int, B: int, nodes: int, expand: int) -> int:
    """bytes of workspace of ``ecbs_device`` (``rmpc_ecbs_work_bytes``)"""
    return _size_query("rmpc_ecbs_work_bytes", H, W, T, B, nodes, expand)


def ecbs_args(grid, start_cell, goal_index, fields, goal_cells, work, paths, status, arrive, info, nodes: int, expand: int,
              rounds: int, w=(11, 10), resume: bool = False, movement: int = 4, occ_threshold: float = 0.8, sep2: int = 9,
              lag: int = 1) -> EcbsArgs:
    """The ``rmpc_ecbs`` of one call: the tensors of ``cbs_args`` with work of ``ecbs_work_bytes`` and info (ECBS_INFO,)
    int32, and the weight ``w = (w_num, w_den)``."""
    a = EcbsArgs()
    a.struct_size = C.sizeof(EcbsArgs)
    a.H, a.W, a.movement = int(grid.shape[0]), int(grid.shape[1]), int(movement)
    a.grid, a.occ_threshold = grid.data_ptr(), float(occ_threshold)
    a.B, a.Gf = int(start_cell.shape[0]), int(fields.shape[0])
    a.start_cell, a.goal_index = start_cell.data_ptr(), goal_index.data_ptr()
    a.fields, a.goal_cells = fields.data_ptr(), goal_cells.data_ptr()
    a.T, a.sep2, a.lag = int(paths.shape[1]) - 1, int(sep2), int(lag)
    a.nodes, a.expand, a.rounds, a.resume = int(nodes), int(expand), int(rounds), int(bool(resume))
    a.work, a.work_bytes = work.data_ptr(), int(work.numel() * work.element_size())
    a.paths, a.status, a.arrive, a.info = paths.data_ptr(), status.data_ptr(), arrive.data_ptr(), info.data_ptr()
    a.w_num, a.w_den = int(w[0]), int(w[1])
    a._keep = (grid, start_cell, goal_index, fields, goal_cells, work, paths, status, arrive, info)
    return a


def ecbs_device(args: EcbsArgs, stream=None):
    """``args.rounds`` rounds of focal conflict-based search over the timed routes, from the root or, with
    ``args.resume``, from the state the workspace holds (``rmpc_ecbs_device``)."""
    _grid_call("rmpc_ecbs_device", C.byref(args), _stream_arg(stream))


class Solver:
    """One handle = one model on one GPU (``rmpc_create`` / ``rmpc_destroy``)."""

    def __init__(self, desc: dict, max_batch: int = 1, device: int = 0):
        self._L = load_library()
        self.desc = desc
        self.cdesc = make_desc(desc, device)
        self.N, self.nx, self.nu, self.ns, self.npar = desc["N"], desc["nx"], desc["nu"], desc["ns"], desc["npar"]
        self.nvar = self.nx + self.ns + self.nu
        self.max_batch = int(max_batch)
        self.device = int(device)
        h = C.c_void_p()
        rc = self._L.rmpc_create(C.byref(self.cdesc), self.max_batch, C.byref(h))
        if rc != 0:
            raise RmpcError("rmpc_create failed: " + self._L.rmpc_last_error().decode())
        self._h = h

    def poison_lds(self):
        """Test aid: NaN patterns into the LDS of every CU (``rmpc_debug_poison_lds``)."""
        self._check(self._L.rmpc_debug_poison_lds(self._h), "rmpc_debug_poison_lds")

    def spec_name(self) -> str:
        """Name of the generated view this handle runs ("" = runtime row tables); ``rmpc_spec_name``."""
        return self._L.rmpc_spec_name(self._h).decode()

    def close(self):
        if getattr(self, "_h", None):
            self._L.rmpc_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != 0:
            raise RmpcError(f"{what} failed: " + self._L.rmpc_last_error().decode())

    def workspace_bytes(self) -> int:
        return int(self._L.rmpc_workspace_bytes(C.byref(self.cdesc), self.max_batch))

    # -- host buffers (numpy) ------------------------------------------------
    def solve(self, xinit, x0, params):
        xinit = np.ascontiguousarray(xinit, dtype=np.float64).reshape(-1, self.nx)
        B = xinit.shape[0]
        x0 = np.ascontiguousarray(x0, dtype=np.float64).reshape(B, self.N * self.nvar)
        params = np.ascontiguousarray(params, dtype=np.float64).reshape(B, self.N * self.npar)
        z = np.empty((B, self.N, self.nvar))
        exitflag = np.empty(B, dtype=np.int32); iters = np.empty(B, dtype=np.int32)
        kkt = np.empty(B); obj = np.empty(B)
        rc = self._L.rmpc_solve_batch(self._h, B, _dp(xinit), _dp(x0), _dp(params), _dp(z), _ip(exitflag),
                                      _ip(iters), _dp(kkt), _dp(obj))
        self._check(rc, "rmpc_solve_batch")
        return dict(z=z, exitflag=exitflag, iters=iters, kkt=kkt, obj=obj)

    # -- device buffers (anything exposing data_ptr(), e.g. torch tensors) ---------
    def solve_device(self, B, xinit, x0, params, z_out, exitflag, iters, kkt, obj, stream=None):
        ptr = lambda t: C.c_void_p(t.data_ptr())
        st = _stream_arg(stream)
        rc = self._L.rmpc_solve_batch_device(self._h, int(B), ptr(xinit), ptr(x0), ptr(params), ptr(z_out),
                                             ptr(exitflag), ptr(iters), ptr(kkt), ptr(obj), st)
        self._check(rc, "rmpc_solve_batch_device")

    # -- scenes and closed loop on the device ----------------------------
    def make_scene(self, weights: dict, dyn_radius: float = 0.1, **tensors) -> RmpcScene:
        """``tensors``: goal, r_body, obst, obst_dyn, lower_limits, upper_limits, lower_limits_u,
        upper_limits_u, lower_limits_vel, upper_limits_vel, lin_constrs -- contiguous fp64 device
        tensors (anything with ``data_ptr()``).  ``weights`` = the YAML ``mpc.weights`` block."""
        s = RmpcScene()
        s.struct_size = C.sizeof(RmpcScene)
        for name, t in tensors.items():
            setattr(s, name, C.c_void_p(t.data_ptr()))
        s.dyn_radius = float(dyn_radius)
        s.w = float(weights.get("w", 0.0)); s.wu = float(weights.get("wu", 0.0)); s.ws = float(weights.get("ws", 0.0))
        wc = list(weights.get("wconstr", []))
        for i in range(MAX_MODULES):
            s.wconstr[i] = float(wc[i]) if i < len(wc) else 0.0
        s._keepalive = tensors  # the struct only holds raw pointers
        return s

    def pack_scene_device(self, B, scene: RmpcScene, params_out, stream=None):
        st = _stream_arg(stream)
        rc = self._L.rmpc_pack_scene_device(self._h, int(B), C.byref(scene), C.c_void_p(params_out.data_ptr()), st)
        self._check(rc, "rmpc_pack_scene_device")

    def solve_scene_device(self, B, scene: RmpcScene, xinit, x0, z_out, exitflag, iters, kkt, obj, stream=None):
        ptr = lambda t: C.c_void_p(t.data_ptr())
        st = _stream_arg(stream)
        rc = self._L.rmpc_solve_batch_scene_device(self._h, int(B), C.byref(scene), ptr(xinit), ptr(x0), ptr(z_out),
                                                   ptr(exitflag), ptr(iters), ptr(kkt), ptr(obj), st)
        self._check(rc, "rmpc_solve_batch_scene_device")

    def pack_scene_workspace(self, B, scene: RmpcScene, stream=None):
        """first half of ``solve_scene_device``: the scene's parameters into the solver's workspace"""
        rc = self._L.rmpc_pack_scene_workspace(self._h, int(B), C.byref(scene), _stream_arg(stream))
        self._check(rc, "rmpc_pack_scene_workspace")

    def solve_packed_device(self, B, xinit, x0, z_out, exitflag, iters, kkt, obj, stream=None):
        """second half: solve with the parameters ``pack_scene_workspace`` left in the workspace"""
        ptr = lambda t: C.c_void_p(t.data_ptr())
        rc = self._L.rmpc_solve_batch_packed_device(self._h, int(B), ptr(xinit), ptr(x0), ptr(z_out), ptr(exitflag), ptr(iters),
                                                    ptr(kkt), ptr(obj), _stream_arg(stream))
        self._check(rc, "rmpc_solve_batch_packed_device")

    def advance_device(self, B, z_prev, xinit, x0, previous_plan: bool, stream=None, exitflag=None):
        """``exitflag`` (device int32 [B], optional): instances whose solve failed restart from their state."""
        st = _stream_arg(stream)
        ef = C.c_void_p(exitflag.data_ptr()) if exitflag is not None else C.c_void_p(0)
        rc = self._L.rmpc_advance_device_flags(self._h, int(B), C.c_void_p(z_prev.data_ptr()), ef,
                                               C.c_void_p(xinit.data_ptr()), C.c_void_p(x0.data_ptr()),
                                               1 if previous_plan else 0, st)
        self._check(rc, "rmpc_advance_device_flags")

    def retarget_device(self, B, xinit, x0, exitflag, goal, goal_pool, cursor, dwell, x_start, tol, max_dwell=0, counts=None,
                        iters=None, mu_regoal=0.0, stream=None, failrun=None, fail_reset_after=0, settle_vel=0.0,
                        settle_min_dwell=0, lower_limits=None, upper_limits=None):
        """Steady closed loop (``rmpc_retarget_device``): next goal from the instance's pool on arrival / coming to rest /
        dwell time-out; a failed solve keeps its state (reset to the start state only after ``fail_reset_after`` failed
        control steps in a row, or at once when it has left the joint-limit box).  All arrays are device tensors;
        ``counts``: int64 [16]."""
        st = _stream_arg(stream)
        p = lambda t: t.data_ptr() if t is not None else None
        a = RetargetArgs()
        a.struct_size = C.sizeof(RetargetArgs)
        a.pool_len = int(goal_pool.shape[1])
        a.xinit, a.x0, a.exitflag, a.iters, a.goal = p(xinit), p(x0), p(exitflag), p(iters), p(goal)
        a.goal_pool, a.x_start, a.cursor, a.dwell, a.failrun = p(goal_pool), p(x_start), p(cursor), p(dwell), p(failrun)
        a.lower_limits, a.upper_limits = p(lower_limits), p(upper_limits)
        a.tol, a.settle_vel, a.mu_regoal = float(tol), float(settle_vel), float(mu_regoal)
        a.settle_min_dwell, a.max_dwell, a.fail_reset_after, a.reserved = int(settle_min_dwell), int(max_dwell), int(fail_reset_after), 0
        a.counts = p(counts)
        rc = self._L.rmpc_retarget_device(self._h, int(B), C.byref(a), st)
        self._check(rc, "rmpc_retarget_device")

    def advance_obstacles_device(self, obst_dyn, dt: float, arena: float = 0.0, stream=None):
        """``rmpc_advance_obstacles_device``: the moving obstacles [B, nobst, 9] one control step on (device tensor)."""
        st = _stream_arg(stream)
        B, nobst = int(obst_dyn.shape[0]), int(obst_dyn.numel() // (9 * obst_dyn.shape[0]))
        rc = self._L.rmpc_advance_obstacles_device(B, nobst, float(dt), float(arena), C.c_void_p(obst_dyn.data_ptr()), st)
        self._check(rc, "rmpc_advance_obstacles_device")

    def set_warm_start(self, enable: bool):
        """Closed loops: start every solve from the multipliers of the previous solve of the same batch
        (``rmpc_set_warm_start``); the plan itself is warm-started through ``x0`` as in the reference."""
        self._check(self._L.rmpc_set_warm_start(self._h, 1 if enable else 0), "rmpc_set_warm_start")

    def set_pass_budget(self, passes: int):
        """Real-time deadline of a solve in passes (``rmpc_set_pass_budget``; 0 = none): instances still iterating
        when it is spent return their last accepted iterate with exit flag 0."""
        self._check(self._L.rmpc_set_pass_budget(self._h, int(passes)), "rmpc_set_pass_budget")

    def is_fused(self) -> bool:
        """True when a solve is one launch that needs no look from the host (``rmpc_is_fused``)."""
        return bool(self._L.rmpc_is_fused(self._h))

    def is_async(self) -> bool:
        """True when a device solve only enqueues work and returns (``rmpc_is_async``): fused handles, and the pass
        kernels under a pass budget."""
        return bool(self._L.rmpc_is_async(self._h))

    def set_profiling(self, enable: bool):
        self._check(self._L.rmpc_set_profiling(self._h, 1 if enable else 0), "rmpc_set_profiling")

    def get_profile(self):
        ms = (C.c_double * NUM_KERNELS)(); n = (C.c_int64 * NUM_KERNELS)()
        by = (C.c_double * NUM_KERNELS)(); full = (C.c_int64 * NUM_KERNELS)()
        self._check(self._L.rmpc_get_profile(self._h, ms, n, by, full), "rmpc_get_profile")
        names = [self._L.rmpc_kernel_name(i).decode() for i in range(NUM_KERNELS)]
        fused = self._L.rmpc_fused_kernel_name(self._h).decode()
        if fused:
            names[NUM_KERNELS - 1] = fused   # ("k_fused" or "k_fused_arm": the kernel this handle's launches run)
        return {names[i]: dict(total_ms=ms[i], launches=n[i], total_alg_bytes=by[i], full_launch_bytes=full[i])
                for i in range(NUM_KERNELS)}

    def fused_stamps(self, nblocks: int):
        out = np.zeros((nblocks, 8), dtype=np.int64)
        self._check(self._L.rmpc_debug_fused_stamps(self._h, out.ctypes.data_as(C.POINTER(C.c_longlong)), nblocks),
                    "rmpc_debug_fused_stamps")
        return out

    def last_passes(self) -> int:
        return int(self._L.rmpc_last_passes(self._h))

    def last_solve_path(self) -> dict:
        """Test aid (``rmpc_last_solve_path``): the kernels the host loop enqueued for the last solve, noted on the host as
        it enqueued them.  ``migrated_at`` (passes enqueued before k_migrate, -1: no migration), ``survivors`` (columns
        moved, -1), ``ric_first`` / ``ric_last`` (``"wave"``, ``"grouped"``, ``"lane"``: recursion kernel of the first
        and of the last pass enqueued), ``compact`` (``"wave"`` or ``"block"``: list builder run on the whole batch) and
        ``fused``; a fused solve, or a handle that has not solved yet, has None for the kernel names."""
        out = (C.c_int32 * 6)()
        self._check(self._L.rmpc_last_solve_path(self._h, out), "rmpc_last_solve_path")
        ric = dict(zip(_k("PATH_RIC_WAVE", "PATH_RIC_GROUPED", "PATH_RIC_LANE"), ("wave", "grouped", "lane")))
        compact = dict(zip(_k("PATH_COMPACT_WAVE", "PATH_COMPACT_BLOCK"), ("wave", "block")))
        return dict(migrated_at=int(out[0]), survivors=int(out[1]), ric_first=ric.get(out[2]), ric_last=ric.get(out[3]),
                    compact=compact.get(out[4]), fused=bool(out[5]))

    def debug_sweep(self, xinit, x0, params):
        xinit = np.ascontiguousarray(xinit, dtype=np.float64).reshape(-1, self.nx)
        B = xinit.shape[0]
        x0 = np.ascontiguousarray(x0, dtype=np.float64).reshape(B, self.N * self.nvar)
        params = np.ascontiguousarray(params, dtype=np.float64).reshape(B, self.N * self.npar)
        nv, N = self.nvar, self.N
        nh = int(self.desc["nh"])
        Q = np.zeros((B, N, nv, nv)); q0 = np.zeros((B, N, nv)); q1 = np.zeros((B, N, nv))
        rc_ = np.zeros((B, N, self.nx)); g = np.zeros((B, N, max(nh, 1))); f = np.zeros((B, N))
        rc = self._L.rmpc_debug_sweep(self._h, B, _dp(xinit), _dp(x0), _dp(params), _dp(Q), _dp(q0), _dp(q1),
                                      _dp(rc_), _dp(g), _dp(f))
        self._check(rc, "rmpc_debug_sweep")
        return dict(Q=Q, q0=q0, q1=q1, rc=rc_, g=g[:, :, :nh], f=f)

    def debug_step(self, xinit, x0, params, duals=None, curv=None):
        """``rmpc_debug_step``: one first sweep and one Riccati recursion on the path this handle runs in production.
        ``duals`` = (lam [B, N, m], nu [B, N, nx], mu [B]) of a previous solve (the warm first pass) or None (cold).
        Returns the blocks the recursion consumed (Q, q0, q1, rc), the slacks, multipliers and barrier parameter they
        were built with (t, lam, mu), the step dz, the new costates nu, the recursion's return value ok and ``path``: what
        the handle holds of the switches that select the path.  ``curv`` = cw (a number, 0.0 included):
        ``rmpc_debug_step_curv`` -- the sweep with the model's curvature terms, the recursion on Q - cw C, and ``C``
        [B, N, nvar, nvar] in the result."""
        xinit = np.ascontiguousarray(xinit, dtype=np.float64).reshape(-1, self.nx)
        B = xinit.shape[0]
        x0 = np.ascontiguousarray(x0, dtype=np.float64).reshape(B, self.N * self.nvar)
        params = np.ascontiguousarray(params, dtype=np.float64).reshape(B, self.N * self.npar)
        nv, N, nx = self.nvar, self.N, self.nx
        # rows of a stage: the general rows, then one per finite lower / upper bound (the library refuses another count)
        m = int(self.desc["nh"]) + sum(int(np.isfinite(float(v))) for bd in ("lb", "ub") for v in self.desc[bd][:nv])
        if duals is None:
            lw = nw = mw = None
        else:
            lw = np.ascontiguousarray(duals[0], dtype=np.float64).reshape(B, N, m)
            nw = np.ascontiguousarray(duals[1], dtype=np.float64).reshape(B, N, nx)
            mw = np.ascontiguousarray(duals[2], dtype=np.float64).reshape(B)
        p = lambda a: _dp(a) if a is not None else None
        Q = np.zeros((B, N, nv, nv)); q0 = np.zeros((B, N, nv)); q1 = np.zeros((B, N, nv)); rc_ = np.zeros((B, N, nx))
        t = np.zeros((B, N, m)); lam = np.zeros((B, N, m)); mu = np.zeros(B)
        dz = np.zeros((B, N, nv)); nu = np.zeros((B, N, nx)); ok = np.zeros(B, dtype=np.int32)
        path = np.zeros(4, dtype=np.int32)
        args = (self._h, B, _dp(xinit), _dp(x0), _dp(params), p(lw), p(nw), p(mw), _dp(Q), _dp(q0),
                _dp(q1), _dp(rc_), _dp(t), _dp(lam), _dp(mu), _dp(dz), _dp(nu),
                ok.ctypes.data_as(C.POINTER(C.c_int32)), m, path.ctypes.data_as(C.POINTER(C.c_int32)))
        extra = {}
        if curv is None:
            rc = self._L.rmpc_debug_step(*args)
        else:
            extra["C"] = np.zeros((B, N, nv, nv))
            rc = self._L.rmpc_debug_step_curv(*args, float(curv), _dp(extra["C"]))
        self._check(rc, "rmpc_debug_step")
        return dict(Q=Q, **extra, q0=q0, q1=q1, rc=rc_, t=t, lam=lam, mu=mu, dz=dz, nu=nu, ok=ok.astype(bool),
                    path=dict(fused=("", "k_fused", "k_fused_arm")[path[0]], ric_lane=int(path[1]), arm_parts=int(path[2]),
                              generated_view=bool(path[3])))
