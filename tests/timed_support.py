"""What the timed planners' test modules share.  For the GPU modules (test_gpu_timed*.py): the runtime, poisoned outputs,
the staging of a case on the device and ``same``.  For the CPU modules (test_timed_*_cpu.py): the library, the fake
pointer of the refusal tables, the checks every header gets, and a struct filled from a dict.  What an entry is launched
with, and what a header declares, stays in the module that tests it."""
import ctypes as C
import math
import os
import re

import numpy as np

from gpu_support import DEV, _t

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POISON = -559038737          # 0xDEADBEEF as an int32
P_ = 0x1000      # a host-side fake pointer: a refusal never dereferences it
I_MAX = 2 ** 31 - 1
NULL = "null argument"


def load_lib():
    import __graft_entry__ as g
    g.build()
    from robot_mpcs_amd import _lib
    return _lib


def load_runtime():
    import torch
    return dict(torch=torch, lib=load_lib())


# ---- the GPU modules ---------------------------------------------------------------------------------------------------
def poisoned(torch, keys, G, B, T, K=1):
    """the outputs ``keys`` of an entry, every element POISON; key is int64, the others int32"""
    shape = dict(paths=(G, B, T + 1), status=(G, B), arrive=(G, B), key=(G,), best=(1,), serve_at=(G, B, K), served=(G, B),
                 unserved=(G,), clash=(B,), order_out=(G, B), rounds_run=(G,), round_best=(G,))
    return {k: torch.full(shape[k], POISON, dtype=torch.int64 if k == "key" else torch.int32, device=DEV) for k in keys}


def workspace(torch, nbytes):
    return torch.full((nbytes,), 0xA5, dtype=torch.uint8, device=DEV)


def stage(rt, grid, cells, orders, movement, occ, stream=None, **int32_inputs):
    """a case on the device -> dict(grid float64, cells, orders (G, B) and every one of ``int32_inputs`` int32, fields):
    fields (len(cells), H, W) starts as NaN and is filled by ``grid_fields_device``, its status starts as POISON"""
    torch, lib = rt["torch"], rt["lib"]
    i32 = torch.int32
    d = dict(grid=_t(torch, np.asarray(grid, dtype=float)), cells=_t(torch, np.asarray(cells, dtype=np.int32), i32),
             orders=_t(torch, np.atleast_2d(np.asarray(orders)).astype(np.int32), i32))
    d.update({k: _t(torch, np.asarray(a), i32) for k, a in int32_inputs.items()})
    d["fields"] = torch.full((len(cells),) + tuple(d["grid"].shape), math.nan, dtype=torch.float64, device=DEV)
    fstat = torch.full((len(cells),), POISON, dtype=i32, device=DEV)
    lib.grid_fields_device(d["grid"], d["cells"], d["fields"], fstat, movement, occ, 3.0, stream=stream)
    return d


def goal_index(goals):
    """(the distinct goal cells, every robot's index into them) as int32"""
    goal_cells = np.unique(np.asarray(goals)).astype(np.int32)
    return goal_cells, np.searchsorted(goal_cells, goals).astype(np.int32)


def same(got, want, keys):
    for k in keys:
        assert np.array_equal(got[k], want[k]), (k, got[k], want[k])


# ---- the CPU modules ---------------------------------------------------------------------------------------------------
def check_header(lib, name, symbols, prototypes):
    """include/``name``.h declares ``symbols`` and nothing else, the loaded library carries ``prototypes`` on them, and
    sources.txt lists the header and its .hpp"""
    code = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", name + ".h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(rmpc_\w+)\s*\(", code))) == sorted(symbols)
    L = lib.load_library()
    for sym in symbols:
        fn = getattr(L, sym)
        assert (fn.restype, list(fn.argtypes)) == tuple(prototypes[sym])
    with open(os.path.join(ROOT, "robot_mpcs_amd", "csrc", "sources.txt")) as f:
        listed = f.read().split()
    assert "include/%s.h" % name in listed and "robot_mpcs_amd/csrc/%s.hpp" % name in listed


def filled(cls, members, **overrides):
    """a ``cls`` with its struct_size, then the members of the dict, then the overrides"""
    a = cls()
    a.struct_size = C.sizeof(cls)
    for k, v in dict(members, **overrides).items():
        setattr(a, k, v)
    return a


def refused(L, rc, want):
    """the call returned -1 and left a message that starts with ``want``"""
    assert rc == -1
    msg = L.rmpc_last_error().decode()
    assert msg.startswith(want) and msg, (msg, want)
