#!/usr/bin/env python3
"""CPU model of k_fused's pass schedule with and without the early hand-over.  No GPU.

The per-instance pass counts of a cfg2 batch come from the oracle (``Oracle.solve_each``: ``passes`` = sweeps of the
solve, line-search retries included -- the oracle counts them).  Which of an instance's passes are retries is not
reported, so the model gives every pass but the last a recursion; the device runs 51.7 k recursions for 56.1 k instance
passes of which 52.0 k are not the last, i.e. the model has 0.6 % recursions too many.

The instances are list-scheduled onto 2 x 1024 half-wavefronts: the first 2048 positions of the queue by the grid, the
others in queue order to whichever half asks first.  "First" needs a clock: a wavefront pass costs the stamped cycles of
the calls it holds (profiles/row_sums_stamps.txt: sweep call 33.5 k for either copy, recursion call 40.2 k, decision
2.5 k, glue 2.2 k, hand-over 6.3 k per site visit), and the wavefronts advance in the order of their clocks.  A dequeue
is booked at the top of the wavefront pass it belongs to, also the early one, which the device makes half a pass
later: the order in which the halves are served is approximate, as the device's own is (it depends on timing).

Two disciplines:
  parent  a half whose instance stops at the decision sits out the partner's recursion and takes its next instance
          at the top of the next wavefront pass
  early   it takes the next instance behind the decision; that instance's first sweep and decision run at once, and its
          first recursion shares the call with the partner's.  At most two rounds per pass.
Two queue orders: by index, and longest first by the true pass count -- the device orders a cold launch by
k_difficulty's estimate, which lies between the two (rmpc_loop.hpp).

Prints, per seed and order: wavefront passes, busy half-passes (instance passes), the busiest wavefront's cycles, the
sum of all wavefronts' cycles, and the ratios early / parent.  ``--json FILE`` writes the same."""
import argparse
import heapq
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SWEEP, RIC, DEC, GLUE, HAND = 33500, 40200, 2500, 2200, 6300   # cycles (profiles/row_sums_stamps.txt, parent)
NWAVE = 1024


def schedule(passes, order, early, nwave=NWAVE):
    """passes [B]: passes per instance; order [B]: queue position -> instance.  Returns a dict of totals."""
    B = len(passes)
    nwave = min(nwave, (B + 1) // 2)
    nxt = 2 * nwave            # the queue counter: positions beyond the grid's own
    left = np.zeros((nwave, 2), dtype=np.int64)     # passes the half's instance still needs (0: none)
    first = np.zeros((nwave, 2), dtype=bool)
    retired = np.zeros((nwave, 2), dtype=bool)
    slot = np.arange(2 * nwave).reshape(nwave, 2)   # queue position of the half's first instance (-1: ask the counter)
    clock = np.zeros(nwave, dtype=np.int64)
    wpasses = busy = both = early_n = recs = 0
    heap = [(0, w) for w in range(nwave)]

    def take(w, h):
        nonlocal nxt
        pos = slot[w, h]
        if pos < 0:
            pos, nxt = nxt, nxt + 1
        slot[w, h] = -1
        if pos < B:
            left[w, h] = passes[order[pos]]
            first[w, h] = True
            return True
        retired[w, h] = True
        return False

    while heap:
        t, w = heapq.heappop(heap)
        # top of the pass: finished instances leave, idle halves take the next instance
        asked = False
        for h in (0, 1):
            if left[w, h] == 0 and not retired[w, h]:
                asked = True
                take(w, h)
        if asked:
            t += HAND
        act = left[w] > 0
        if not act.any():
            clock[w] = t
            continue
        wpasses += 1
        busy += int(act.sum())
        f = first[w] & act
        if f.any() and (act & ~f).any():
            both += 1
            t += SWEEP
        t += SWEEP + DEC + GLUE
        left[w][act] -= 1
        first[w][act] = False
        if early:
            stopped = act & (left[w] == 0)
            if stopped.any():
                t += HAND
                got = False
                for h in (0, 1):
                    if stopped[h]:
                        early_n += 1
                        if take(w, h):
                            got = True
                            busy += 1
                            left[w, h] -= 1
                            first[w, h] = False
                if got:
                    t += SWEEP + DEC
        if (left[w] > 0).any():
            recs += int((left[w] > 0).sum())
            t += RIC
        heapq.heappush(heap, (t, w))
    return dict(wavefront_passes=int(wpasses), busy_half_passes=int(busy), both_copies=int(both),
                early_handovers=int(early_n), recursions=int(recs), max_cycles=int(clock.max()),
                sum_cycles=int(clock.sum()))


def pass_counts(seed, B):
    from oracle.oracle import Oracle
    from robot_mpcs_amd.scenarios import make_scenario
    sc = make_scenario("cfg2", B=B, seed=seed)
    r = Oracle(sc.desc).solve_each(sc.xinit, sc.x0, sc.params)
    return np.asarray(r["passes"], dtype=np.int64), np.asarray(r["iters"], dtype=np.int64)


def model_seed(arg):
    seed, B = arg
    p, it = pass_counts(seed, B)
    out = dict(seed=seed, B=B, passes_mean=float(p.mean()), passes_max=int(p.max()),
               retries=int((p - it - 1).sum()))
    for name, order in (("index", np.arange(B)), ("longest_first", np.argsort(-p, kind="stable"))):
        a, b = schedule(p, order, False), schedule(p, order, True)
        out[name] = dict(parent=a, early=b,
                         ratio_wavefront_passes=b["wavefront_passes"] / a["wavefront_passes"],
                         ratio_max_cycles=b["max_cycles"] / a["max_cycles"],
                         ratio_sum_cycles=b["sum_cycles"] / a["sum_cycles"])
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--seeds", type=int, nargs="*",
                    default=[1000 + 17 * i for i in range(6)] + [3, 500, 2024])   # bench.py's six sets and three others
    ap.add_argument("--jobs", type=int, default=min(9, os.cpu_count() or 1))
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    import __graft_entry__ as g
    from oracle import oracle as orc
    orc.build()
    del g
    import multiprocessing as mp
    with mp.get_context("fork").Pool(args.jobs) as pool:
        rows = pool.map(model_seed, [(s, args.batch) for s in args.seeds])
    for r in rows:
        print(f"seed {r['seed']} B={r['B']}: passes per instance mean {r['passes_mean']:.2f} max {r['passes_max']}, "
              f"line-search retries {r['retries']}")
        for name in ("index", "longest_first"):
            o = r[name]
            for side in ("parent", "early"):
                d = o[side]
                print(f"  {name:13s} {side:6s} wavefront passes {d['wavefront_passes']:6d}  busy half-passes "
                      f"{d['busy_half_passes']:6d}  per wavefront pass {d['busy_half_passes'] / d['wavefront_passes']:.3f}  "
                      f"early hand-overs {d['early_handovers']:5d}  cycles max {d['max_cycles']:8d} sum {d['sum_cycles']:11d}")
            print(f"  {name:13s} early / parent: wavefront passes {o['ratio_wavefront_passes']:.4f}, "
                  f"busiest wavefront {o['ratio_max_cycles']:.4f}, all wavefronts {o['ratio_sum_cycles']:.4f}")
    mean = {name: {k: float(np.mean([r[name][k] for r in rows]))
                   for k in ("ratio_wavefront_passes", "ratio_max_cycles", "ratio_sum_cycles")}
            for name in ("index", "longest_first")}
    print("mean of the seeds:", json.dumps(mean))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(dict(what="scripts/early_handover_model.py: list schedule of cfg2 batches on 2 x 1024 half-wavefronts, "
                                "parent discipline against the early hand-over; pass counts from the oracle (retries "
                                "included); cycles per call from profiles/row_sums_stamps.txt",
                           cycles=dict(sweep=SWEEP, recursion=RIC, decide=DEC, glue=GLUE, hand_over=HAND),
                           seeds=rows, mean_of_seeds=mean), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
