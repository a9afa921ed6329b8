"""Search for the witnesses of tests/decision_cases.py (CPU only, the oracle; minutes).

    python tests/tools/find_decision_cases.py [--seeds 12] [--jobs 8]

Scans scenario x seed x mode (cold, cold with mu0 = 1e-2, warm, warm-disturbed at 0.1 and 0.3) with batches of 16 and up
to 5 control steps, takes the oracle's branch census of every solve, and prints per (model class, branch) the cheapest
witnesses -- fewest passes first, among instances that finish within decision_cases.MAX_PASSES passes and pass the
rounding filter (decision_cases.rounding_insensitive) -- and then a small set of cases that covers every pair, as
``Case(...)`` lines for decision_cases.CASES, with the pairs it could not reach and the number of instances searched.
"""
import argparse
import multiprocessing as mp
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import decision_cases as dc  # noqa: E402

B, STEPS = 16, 5
# (class, group, scenario, overrides): group "+": not needed for completeness, searched for the kernel paths only that
# class's other scenarios do not reach (ric_backward; a horizon of 40 stages)
SCENARIOS = [
    ("chain3", "", "cfg2", {}), ("chain3", "", "chain2", {}), ("chain3", "", "wc_point", {}), ("chain3", "+N40", "cfg2", {"time_horizon": 40}),
    ("point_slack", "", "cfg2", {"slack": True}),
    ("unicycle", "", "cfg3", {}), ("unicycle", "", "boxer", {}), ("unicycle", "", "wc_boxer", {}), ("unicycle", "+slack", "wc_boxer_slack", {}),
    ("arm", "", "cfg4", {}), ("arm", "", "chain5", {}), ("arm", "", "chain6", {}),
    ("arm", "+dense", "chain4", {}), ("arm", "+dense", "chain8", {}),
]
MODES = [("cold", 0.0, {}), ("cold", 0.0, {"mu0": 1e-2}), ("warm", 0.0, {}), ("disturbed", 0.1, {}), ("disturbed", 0.3, {})]


def scan(job):
    """One loop: [(class, group, branch, passes, Case)] of every solve that takes a branch, and the instances solved."""
    from oracle.oracle import Oracle
    from robot_mpcs_amd.scenarios import make_scenario
    cls, group, name, kw, seed, (mode, scale, opts) = job
    steps = 1 if mode == "cold" else STEPS
    c = dc.Case(cls, name, kw, opts, seed, B, steps, mode, scale, 0, ())
    sc = dc.scenario_of(make_scenario, c)
    o = Oracle(sc.desc)
    loop = dc.oracle_loop(sc, o, c)
    found = []
    for t, step in enumerate(loop):
        if mode != "cold" and t == 0:
            continue   # (the first step of a loop is the cold solve)
        cpu = step["cpu"]
        for b in range(B):
            if cpu["passes"][b] > dc.MAX_PASSES or cpu["exitflag"][b] == 0:
                continue
            took = tuple(k for k, f in dc.BRANCHES.items() if f(cpu["census"][b]))
            cand = c._replace(steps=t + 1, witness=b, branches=took)
            for k in took:
                found.append((cls, group, k, int(cpu["passes"][b]), cand))
    return found, B * len(loop)


def _k(cand):
    return (dc.case_id(cand), cand.steps)


def robust(cand):
    from oracle.oracle import Oracle
    from robot_mpcs_amd.scenarios import make_scenario
    sc = dc.scenario_of(make_scenario, cand)
    o = Oracle(sc.desc)
    loop = dc.oracle_loop(sc, o, cand)
    return dc.rounding_insensitive(o, sc, cand, loop[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=12)
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("--keep", type=int, default=3, help="robust witnesses kept per (class, group, branch)")
    a = ap.parse_args()
    jobs = [(cls, g, n, kw, seed, m) for cls, g, n, kw in SCENARIOS for seed in range(1, a.seeds + 1) for m in MODES]
    os.environ.setdefault("OMP_NUM_THREADS", "1")
    with mp.Pool(a.jobs) as pool:
        res = pool.map(scan, jobs, chunksize=1)
        searched, cands = {}, {}
        for (found, n), job in zip(res, jobs):
            searched[(job[0], job[1])] = searched.get((job[0], job[1]), 0) + n
            for cls, g, k, p, cand in found:
                cands.setdefault((cls, g, k), []).append((p, cand))
        # rounding filter, cheapest first, until `keep` witnesses of a pair have passed it
        kept, verdict = {}, {}
        for key in sorted(cands):
            lst = sorted(cands[key], key=lambda pc: (pc[0], pc[1].steps, pc[1].seed))
            kept[key] = []
            for i in range(0, min(len(lst), 24), a.jobs):
                chunk = [pc for pc in lst[i:i + a.jobs]]
                todo = [pc[1] for pc in chunk if _k(pc[1]) not in verdict]
                for cand, ok in zip(todo, pool.map(robust, todo, chunksize=1)):
                    verdict[_k(cand)] = ok
                kept[key] += [pc for pc in chunk if verdict[_k(pc[1])]]
                if len(kept[key]) >= a.keep:
                    break
            kept[key] = kept[key][:a.keep]
    print("# cheapest rounding-insensitive witnesses per (class, group, branch): passes, case")
    for key in sorted(kept):
        for p, cand in kept[key]:
            print("#   %-12s %-7s %-14s %3d  %s" % (key + (p, dc.case_id(cand))))
    # a small cover: per (class, group), greedily the witness that takes most of the branches still open
    print("CASES = [")
    for cls, g in sorted(searched):
        want = {k for k in dc.BRANCHES if (cls, k) not in dc.NOT_APPLICABLE and kept.get((cls, g, k))}
        pool_ = {_k(cand): (p, cand) for k in want for p, cand in kept[(cls, g, k)]}
        while want:
            p, cand = max(pool_.values(), key=lambda pc: (len(want & set(pc[1].branches)), -pc[0]))
            print("    Case(%r, %r, %r, %r, %d, %d, %d, %r, %r, %d, %r),   # %d passes%s" % (
                cand.cls, cand.name, cand.kw, cand.opts, cand.seed, cand.B, cand.steps, cand.mode, cand.scale, cand.witness,
                tuple(sorted(want & set(cand.branches))), p, " (%s)" % g if g else ""))
            want -= set(cand.branches)
    print("]")
    print("UNREACHED = {")
    for cls in dc.CLASSES:
        n = sum(v for (c_, g), v in searched.items() if c_ == cls)
        for k in dc.BRANCHES:
            if (cls, k) not in dc.NOT_APPLICABLE and not any(kept.get((cls, g, k)) for (c_, g) in searched if c_ == cls):
                print("    (%r, %r): %d,%s" % (cls, k, n, "" if any((cls, g, k) in cands for (c_, g) in searched if c_ == cls)
                                               else "   # (never seen, rounding filter aside)"))
    print("}")


if __name__ == "__main__":
    main()
