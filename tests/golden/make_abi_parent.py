"""Records tests/golden/abi_parent.json: the ctypes binding of robot_mpcs_amd/_lib.py as the commit before the binding
was derived from include/rmpc.h wrote it down by hand -- restype and argtypes of every function, the layout of the ten
structs, the limits and codes, the decoding of ``Solver.last_solve_path`` and the public names.  Run at that commit:

    python tests/golden/make_abi_parent.py tests/golden/abi_parent.json

It needs no library and no GPU: ``ctypes.CDLL`` is a recorder while ``load_library()`` runs.  tests/test_abi.py takes
``record()`` from here, applies it to the library it has loaded and holds the result to the file entry for entry.
"""
import ctypes as C
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# Python name in _lib -> struct of include/rmpc.h
STRUCTS = {"RmpcDesc": "rmpc_desc", "RmpcScene": "rmpc_scene", "RetargetArgs": "rmpc_retarget", "LidarArgs": "rmpc_lidar",
           "LidarBodiesArgs": "rmpc_lidar_bodies", "GridMarkArgs": "rmpc_grid_mark", "ScanMatchArgs": "rmpc_scan_match",
           "ScanSearchArgs": "rmpc_scan_search", "TracksArgs": "rmpc_tracks", "TimedPlanArgs": "rmpc_timed_plan"}
CONSTANTS = ["MAX_JOINTS", "MAX_LINKS", "MAX_PAIRS", "MAX_MODULES", "NV_MAX", "MAX_XROWS", "NUM_KERNELS",
             "GRID_MAX_CELLS", "GRID_OK", "GRID_START_OCCUPIED", "GRID_GOAL_OCCUPIED", "GRID_OUTSIDE", "GRID_TOO_LONG",
             "GRID_BAD_MAP", "GRID_NO_FIXED_POINT", "GRID_BAD_SEED", "ASSIGN_MAX_ROBOTS", "ASSIGN_MAX_TARGETS",
             "MATCH_MAX_RAYS", "MATCH_MAX_N", "SEARCH_MAX_N", "SEARCH_MAX_TOP", "SEARCH_MAX_LEVELS", "LIDAR_FLEET_LIST",
             "TRACK_MAX_RAYS", "TRACK_MAX_TRACKS", "TRACK_MAX_DET", "TIMED_MAX_ROBOTS", "TIMED_MAX_T", "TIMED_MAX_ORDERS",
             "TIMED_MAX_SEP2", "TIMED_MAX_LAG", "TIMED_BAD_ORDER"]


def spell(t, cname) -> str:
    """A ctypes type by its class name (c_int32 is c_int, c_int64 is c_long), a pointer as ptr:<pointee>, the pointee
    by its C name when it is one of the structs."""
    if t is None:
        return "None"
    if issubclass(t, C._Pointer):
        return "ptr:" + cname.get(t._type_, t._type_.__name__)
    return t.__name__


def solve_path_decoding(_lib) -> dict:
    """What ``Solver.last_solve_path`` makes of each code -1 .. 3 in the words 2, 3 and 4: [ric_first, ric_last, compact]."""
    out = {}
    for code in range(-1, 4):
        def fill(h, words, code=code):
            words[2] = words[3] = words[4] = code
            return 0
        me = types.SimpleNamespace(_L=types.SimpleNamespace(rmpc_last_solve_path=fill), _h=None,
                                   _check=lambda rc, what: None)
        r = _lib.Solver.last_solve_path(me)
        out[str(code)] = [r["ric_first"], r["ric_last"], r["compact"]]
    return out


def record(_lib, L) -> dict:
    """The binding of the module ``_lib`` with the declarations found on ``L`` (what ``load_library()`` returned).
    A function whose argtypes nobody set has the argument list [], which is how the hand-written binding left the
    functions that take none."""
    cname = {getattr(_lib, py): c for py, c in STRUCTS.items()}
    functions = {}
    for name in sorted(_lib.EXPORTED_SYMBOLS):
        fn = getattr(L, name)
        functions[name] = [spell(fn.restype, cname), [spell(a, cname) for a in fn.argtypes or ()]]
    structs = {}
    for cls, c in cname.items():
        rows = [[f, getattr(cls, f).offset, getattr(cls, f).size, t.__name__] for f, t in cls._fields_]
        structs[c] = dict(size=C.sizeof(cls), fields=rows)
    return dict(functions=functions, structs=structs, constants={n: getattr(_lib, n) for n in CONSTANTS},
                solve_path=solve_path_decoding(_lib), public=sorted(n for n in vars(_lib) if not n.startswith("_")))


class _Function:
    restype, argtypes = C.c_int, None      # what ctypes assumes of a function nothing was declared for

    def __init__(self, result):
        self.result = result

    def __call__(self, *args):
        return self.result


def main():
    sys.path.insert(0, ROOT)
    from robot_mpcs_amd import _lib

    class Recorder:
        def __init__(self, path):
            self.rmpc_desc_size = _Function(C.sizeof(_lib.RmpcDesc))    # the one call load_library() checks

        def __getattr__(self, name):
            setattr(self, name, _Function(0))
            return self.__dict__[name]

    try:
        import torch  # noqa: F401  (load_library() imports it, and it loads its own libraries through ctypes.CDLL)
    except ImportError:
        pass
    os.environ["RMPC_ALLOW_STALE"] = "1"      # nothing was built: there is no hash to compare
    real, C.CDLL, _lib._lib = C.CDLL, Recorder, None
    try:
        L = _lib.load_library(os.path.abspath(__file__))
    finally:
        C.CDLL, _lib._lib = real, None
    parts = []                                # one line per function, struct and constant
    for section, body in sorted(record(_lib, L).items()):
        if isinstance(body, dict):
            rows = ",\n".join("  %s: %s" % (json.dumps(k), json.dumps(v, sort_keys=True)) for k, v in sorted(body.items()))
            parts.append(" %s: {\n%s\n }" % (json.dumps(section), rows))
        else:
            parts.append(" %s: %s" % (json.dumps(section), json.dumps(body)))
    with open(sys.argv[1], "w") as f:
        f.write("{\n" + ",\n".join(parts) + "\n}\n")


if __name__ == "__main__":
    main()
