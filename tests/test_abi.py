"""The C-ABI library loads on a machine without a GPU and exports every symbol
include/rmpc.h declares; product code fails loudly without a device.  CPU only."""
import ctypes as C
import importlib.util
import json
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from robot_mpcs_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def abi(lib):
    from robot_mpcs_amd import _abi
    return _abi


def test_every_declared_symbol_is_exported(lib, abi):
    declared = set(abi.prototypes)
    assert declared, "no declarations parsed"
    L = C.CDLL(lib.LIB_PATH)
    for sym in sorted(declared):
        assert hasattr(L, sym), f"{sym} declared in include/rmpc.h but not exported"
    assert declared == set(lib.EXPORTED_SYMBOLS)
    # the reader has dropped no prototype: a plain count of the names in the header's code agrees
    code = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "rmpc.h")).read(), flags=re.S)
    names = re.findall(r"\b(rmpc_[a-z_]+)\s*\(", code)
    assert len(names) == len(set(names)) == len(abi.prototypes) and set(names) == declared


def test_descriptor_layout_and_version(lib, abi):
    L = lib.load_library()
    assert L.rmpc_desc_size() == C.sizeof(lib.RmpcDesc)
    # the macro of include/rmpc.h is what the library reports (0.2.0: rmpc_retarget struct, rmpc_advance_obstacles_device)
    assert L.rmpc_version() == abi.constants["RMPC_VERSION"] == 201
    assert [L.rmpc_kernel_name(i).decode() for i in range(5)] == ["k_pack", "k_sweep", "k_riccati", "k_step", "k_unpack"]


def test_debug_step_hooks_are_exported_and_refuse_a_null_handle(lib):
    """rmpc_debug_step and rmpc_debug_step_curv (the same hook with the curvature weight and out_C) are part of the
    exported set and fail cleanly without a handle."""
    L = lib.load_library()
    assert {"rmpc_debug_step", "rmpc_debug_step_curv"} <= set(lib.EXPORTED_SYMBOLS)
    assert len(L.rmpc_debug_step_curv.argtypes) == len(L.rmpc_debug_step.argtypes) + 2
    none = [None] * 15
    i32 = C.POINTER(C.c_int32)()
    assert L.rmpc_debug_step(None, 1, *none, i32, 0, i32) != 0
    assert L.rmpc_debug_step_curv(None, 1, *none, i32, 0, i32, 1.0, None) != 0
    assert b"null" in L.rmpc_last_error()


def test_last_solve_path_is_exported_and_refuses_a_null_handle(lib, abi):
    """rmpc_last_solve_path (which kernels the host loop enqueued for the last solve) is part of the exported set and fails
    cleanly without a handle, leaving the caller's words alone; the codes it returns are the header's."""
    L = lib.load_library()
    assert "rmpc_last_solve_path" in lib.EXPORTED_SYMBOLS
    out = (C.c_int32 * 6)(*([77] * 6))
    assert L.rmpc_last_solve_path(None, out) != 0
    assert b"null" in L.rmpc_last_error()
    assert list(out) == [77] * 6
    codes = {k: v for k, v in abi.constants.items() if k.startswith("RMPC_PATH_")}
    assert codes == {"RMPC_PATH_RIC_WAVE": 0, "RMPC_PATH_RIC_GROUPED": 1, "RMPC_PATH_RIC_LANE": 2,
                     "RMPC_PATH_COMPACT_WAVE": 0, "RMPC_PATH_COMPACT_BLOCK": 1}   # (what Solver.last_solve_path decodes)


def test_binding_is_what_the_hand_written_one_was(lib):
    """restype and argtypes as the loaded library carries them, the layout of the ten structs, the limits and codes and
    the decoding of last_solve_path equal, entry for entry, what the last hand-written _lib.py declared
    (tests/golden/abi_parent.json, recorded by tests/golden/make_abi_parent.py at that commit); every public name of
    that _lib still exists."""
    spec = importlib.util.spec_from_file_location("make_abi_parent", os.path.join(GOLDEN, "make_abi_parent.py"))
    rec = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rec)
    with open(os.path.join(GOLDEN, "abi_parent.json")) as f:
        want = json.load(f)
    got = json.loads(json.dumps(rec.record(lib, lib.load_library())))      # (tuples as lists, keys as strings)
    assert len(want["functions"]) == 65 and len(want["structs"]) == 10
    for section in ("functions", "structs", "constants", "solve_path"):
        assert set(got[section]) == set(want[section]), section
        for key in want[section]:
            assert got[section][key] == want[section][key], (section, key)
    assert set(want["public"]) <= set(got["public"]), sorted(set(want["public"]) - set(got["public"]))


SIZED = [("rmpc_lidar", "rmpc_lidar_scan_device"), ("rmpc_lidar_bodies", "rmpc_lidar_scan_fleet_device"),
         ("rmpc_grid_mark", "rmpc_grid_mark_device"), ("rmpc_scan_match", "rmpc_scan_match_device"),
         ("rmpc_scan_search", "rmpc_scan_search_device"), ("rmpc_tracks", "rmpc_lidar_tracks_device"),
         ("rmpc_timed_plan", "rmpc_timed_plan_device")]


@pytest.mark.parametrize("cname,entry", SIZED)
def test_struct_sizes_are_the_compilers(lib, abi, cname, entry):
    """The size Python derives for a struct is the library's sizeof: the struct's entry refuses a wrong struct_size
    before it looks at anything else or touches a device, so a zeroed struct with B = 0 fails either way, and only the
    wrong size fails on the size.  rmpc_desc has rmpc_desc_size() (test_descriptor_layout_and_version); rmpc_scene and
    rmpc_retarget sit behind a handle, their size is checked by the first call of the GPU tests that pass one."""
    L = lib.load_library()
    cls = abi.structs[cname]

    def refusal(size):
        s = cls()
        s.struct_size = size
        if cname == "rmpc_timed_plan":
            rc = L.rmpc_timed_plan_device(C.byref(s), None)
        elif cname == "rmpc_lidar_bodies":
            scan = abi.structs["rmpc_lidar"]()
            scan.struct_size = C.sizeof(scan)
            rc = L.rmpc_lidar_scan_fleet_device(0, C.byref(scan), C.byref(s), None)
        else:
            rc = getattr(L, entry)(0, C.byref(s), None)
        assert rc != 0
        return L.rmpc_last_error().decode()

    assert "struct_size mismatch" not in refusal(C.sizeof(cls))
    assert cname + ".struct_size mismatch" in refusal(C.sizeof(cls) - 4)


HEADER = """
#ifndef RMPC_H
#define RMPC_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define RMPC_MAX_JOINTS 8
#define RMPC_BAD (-3)   /* a status */
typedef struct rmpc_pod {
  int32_t struct_size;   /* sizeof(rmpc_pod) */
  double m[RMPC_MAX_JOINTS][3];
  int32_t *a, *b;
  const double *pose; int32_t pose_stride;
  double x0, y0, cell;
  int64_t *counts;
} rmpc_pod;
typedef struct rmpc_handle rmpc_handle;
/* a comment that holds rmpc_foo(int x); and a second ; */
int rmpc_create(const rmpc_pod *p,
                int max_batch,
                rmpc_handle **out);
int rmpc_path(const rmpc_handle *h, int32_t out[6]);
const char *rmpc_name(void);
void rmpc_run(rmpc_handle *h, const double *xinit, const double *d_xinit, long long *stamps, const char *name, char *buf,
              int64_t cap, void *stream);
%s
#ifdef __cplusplus
}
#endif
#endif
"""


def test_reader_types_the_forms_of_the_header(abi):
    constants, structs, prototypes = abi.parse(HEADER % "")
    assert constants == {"RMPC_MAX_JOINTS": 8, "RMPC_BAD": -3}
    pod = structs["rmpc_pod"]
    assert list(structs) == ["rmpc_pod"] and issubclass(pod, C.Structure)
    assert pod._fields_ == [("struct_size", C.c_int32), ("m", (C.c_double * 3) * 8), ("a", C.c_void_p), ("b", C.c_void_p),
                            ("pose", C.c_void_p), ("pose_stride", C.c_int32), ("x0", C.c_double), ("y0", C.c_double),
                            ("cell", C.c_double), ("counts", C.c_void_p)]
    assert C.sizeof(pod) == 8 + 8 * 3 * 8 + 8 + 8 + 8 + 8 + 3 * 8 + 8
    dp = C.POINTER(C.c_double)
    assert prototypes == {      # the prototype over three lines, out[6], rmpc_handle **, and no rmpc_foo from the comment
        "rmpc_create": (C.c_int, [C.POINTER(pod), C.c_int, C.POINTER(C.c_void_p)]),
        "rmpc_path": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]),
        "rmpc_name": (C.c_char_p, []),
        "rmpc_run": (None, [C.c_void_p, dp, C.c_void_p, C.POINTER(C.c_longlong), C.c_char_p, C.c_char_p, C.c_int64,
                            C.c_void_p])}


@pytest.mark.parametrize("line,names", [
    ("int rmpc_resize(rmpc_handle *h, unsigned n);", "unsigned n"),
    ("int rmpc_watch(rmpc_handle *h, int (*cb)(int));", "(*cb)"),
    ("typedef struct rmpc_bits { int32_t struct_size; int32_t flags : 3; } rmpc_bits;", "flags : 3"),
    ("typedef union rmpc_either { int32_t i; double d; } rmpc_either;", "union rmpc_either"),
    ("typedef struct rmpc_rows { double lb[RMPC_NOT_DEFINED]; } rmpc_rows;", "RMPC_NOT_DEFINED"),
    ("extern int rmpc_counter;", "extern int rmpc_counter"),
])
def test_reader_refuses_what_it_does_not_understand(abi, line, names):
    with pytest.raises(abi.RmpcError) as e:
        abi.parse(HEADER % line)
    assert names in str(e.value)


def test_workspace_bytes_is_host_only_and_scales(lib):
    from robot_mpcs_amd.scenarios import make_scenario
    L = lib.load_library()
    sc = make_scenario("cfg2", B=1)
    d = lib.make_desc(sc.desc)
    w1 = L.rmpc_workspace_bytes(C.byref(d), 64)
    w2 = L.rmpc_workspace_bytes(C.byref(d), 4096)
    assert 0 < w1 < w2
    assert w2 < 2 * 64 * w1
    # cfg2 at B = 4096: a few hundred MB, far below 288 GB of HBM
    assert 100e6 < w2 < 1e9


def test_invalid_descriptors_are_rejected(lib):
    from robot_mpcs_amd.scenarios import make_scenario
    L = lib.load_library()
    sc = make_scenario("cfg1", B=1)
    d = lib.make_desc(sc.desc)
    d.struct_size = 4
    assert L.rmpc_workspace_bytes(C.byref(d), 8) == -1
    d = lib.make_desc(sc.desc)
    d.off_goal = 10_000
    assert L.rmpc_workspace_bytes(C.byref(d), 8) == -1
    assert b"goal" in L.rmpc_last_error()
    d = lib.make_desc(sc.desc)
    d.module_kind[0] = 77
    assert L.rmpc_workspace_bytes(C.byref(d), 8) == -1


def test_no_silent_cpu_fallback(lib):
    """Without a HIP device the product raises; it never routes to the oracle."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from robot_mpcs_amd.scenarios import make_scenario
    sc = make_scenario("cfg1", B=1)
    with pytest.raises(lib.RmpcError):
        lib.Solver(sc.desc, max_batch=1)


def test_product_never_imports_oracle():
    pkg = os.path.join(ROOT, "robot_mpcs_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".hpp", ".h")):
                src = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", src, re.M), f
                assert not re.search(r"#\s*include\s*[<\"][^>\"]*oracle", src), f
                assert "librmpc_oracle" not in src and "rmpc_oracle.h" not in src, f
