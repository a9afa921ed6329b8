#!/usr/bin/env python3
"""Development aid: phase breakdown of the fused kernel (library built with -DRMPC_STAMPS, RMPC_LIB_PATH set).
With -DRMPC_STAMPS_CALLS_ONLY beside it the sweep call carries no section stamps and the section lines are left out:
the phase figures are then those of the calls as a production build runs them (rmpc_stamps.hpp)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from robot_mpcs_amd._lib import Solver  # noqa: E402
from robot_mpcs_amd.scenarios import DEFAULT_BATCH, make_scenario  # noqa: E402

cfg = sys.argv[1] if len(sys.argv) > 1 else "cfg2"
B = int(sys.argv[2]) if len(sys.argv) > 2 else DEFAULT_BATCH[cfg]
sc = make_scenario(cfg, B=B, seed=1000)
s = Solver(sc.desc, max_batch=B)
s.solve(sc.xinit, sc.x0, sc.params)
r = s.solve(sc.xinit, sc.x0, sc.params)
# the launch is a queue drained by at most one wavefront per SIMD (4 x compute units; RMPC_FUSED_GRID overrides)
nb = min((B + 1) // 2, int(os.environ.get("RMPC_FUSED_GRID", "1024")))
both = s.fused_stamps(2 * nb)
st, sec = both[:nb].astype(float), both[nb:].astype(float)
# word 5 of a wavefront's record: its passes (low half) and how many of them ran both copies of the sweep call, the one
# for an instance's first pass and the one for the others, because its two halves differed (bits 32 .. 47), and its early
# hand-overs: epilogues at the site behind the decision, round 1 of a pass (bits 48 .. 63; a library from before that
# site leaves them 0)
raw5 = both[:nb, 5].astype(np.int64)
st[:, 5] = (raw5 & 0xffffffff).astype(float)
double_sweeps = ((raw5 >> 32) & 0xffff).astype(float)
early = ((raw5 >> 48) & 0xffff).astype(float)
# word 7: instance passes of the wavefront (low half) and its hand-over events, epilogues + prologues (high half; a
# library from before the hand-over stamp leaves it 0 and keeps a time stamp in word 6)
raw7 = both[:nb, 7].astype(np.int64)
st[:, 7] = (raw7 & 0xffffffff).astype(float)
handovers = (raw7 >> 32).astype(float)
tot = st[:, 4]
print(f"{cfg} B={B}: wavefronts {len(st)}, passes per wavefront mean {st[:, 5].mean():.1f} max {st[:, 5].max():.0f}, "
      f"instance passes per wavefront pass {st[:, 7].sum() / st[:, 5].sum():.2f} (2 = both halves busy; an early hand-over "
      f"adds the first pass of the instance it takes), "
      f"passes per instance mean {st[:, 7].sum() / B:.1f}")
for i, name in enumerate(["sweep", "decide", "riccati", "step"]):
    print(f"  {name:8s} {st[:, i].sum() / tot.sum() * 100:5.1f} %   cycles per pass {st[:, i].sum() / st[:, 5].sum():9.0f}")
if sec[:, :6].sum() > 0:
    # generated views (merged call): the stage's requests leave once, in section 5, which also forms the step lengths
    # from them; section 1 is then the trial point alone.  Runtime tables: section 1 holds the top loads, 5 and 6 are empty.
    for i, name in enumerate(["trial point (runtime tables: + top loads)", "objective, kinematics, distance rows", "single-variable rows", "dynamics, records, log",
                              "top loads + step lengths (merged call)", "reduction of the step lengths", "after the call: unpark + reductions", "ordering point (wait for the stores)"]):
        print(f"     sweep / {name:42s} {sec[:, i].sum() / st[:, 5].sum():9.0f}")
    print(f"  wavefront passes with both copies of the sweep call: {double_sweeps.sum():.0f} of {st[:, 5].sum():.0f} "
          f"({double_sweeps.sum() / st[:, 5].sum() * 100:.2f} %), per wavefront {double_sweeps.mean():.2f}")
passes = st[:, 5].sum()
print(f"  outside the four phases (total minus their sum): cycles per pass {(tot.sum() - st[:, :4].sum()) / passes:.0f}")
if handovers.sum() > 0:
    # stamped: from the top of a round of the pass loop to the test that ends it (epilogue, dequeue, prologue and its
    # ordering point), both sites: the top of the pass and the early one behind the decision
    print(f"  hand-over: cycles per pass {st[:, 6].sum() / passes:.0f}, cycles per event {st[:, 6].sum() / handovers.sum():.0f} "
          f"({handovers.sum():.0f} events, {handovers.mean():.1f} per wavefront)")
    print(f"  early hand-overs (epilogues behind the decision): {early.sum():.0f}, per wavefront {early.mean():.2f}")
if sec[:, :6].sum() == 0:
    print(f"  wavefront passes with both copies of the sweep call: {double_sweeps.sum():.0f} of {passes:.0f} "
          f"({double_sweeps.sum() / passes * 100:.2f} %)")
print(f"  total cycles per pass {tot.sum() / passes:.0f}   (s_memtime: shader clock)")
print(f"  total cycles per wavefront (passes x cycles per pass) mean {tot.mean():.0f} max {tot.max():.0f}")
