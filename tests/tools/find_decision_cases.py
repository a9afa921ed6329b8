"""Search for the witnesses of tests/decision_cases.py (CPU only, the oracle; minutes).

    python tests/tools/find_decision_cases.py [--seeds 12] [--opt-seeds 4] [--jobs 8] [--part all|default|options|edges]

Default options: scans scenario x seed x mode (cold, cold with mu0 = 1e-2, warm, warm-disturbed at 0.1 and 0.3) with
batches of 16 and up to 5 control steps, takes the oracle's branch census of every solve, and prints per (model class,
branch) the cheapest witnesses -- fewest passes first, among instances that finish within decision_cases.MAX_PASSES
passes and pass the rounding filter (decision_cases.rounding_insensitive) -- and then a small set of cases that covers
every pair, as ``Case(...)`` lines for decision_cases.CASES, with the pairs it could not reach and the number of
instances searched.

Option sets (decision_cases.OPTION_SETS: ACC, ACC_OFF, BENCH, LS, LOOSE), each in the modes cold, warm and disturbed at
0.1 and 0.3: the same scan over the first --opt-seeds seeds, for the exits decision_cases.OPTION_BRANCHES names per set
(under LOOSE the default-tolerance solve of the same inputs is computed beside it).  Per (class, group) one case per
branch, the cheapest; ACC_OFF is listed only (its flag-1 solves: what goes on where the default window would have
stopped); per class without a cold flag-2 case at the default options, the cheapest cold one (for the max_iter
edge); and per class the cheapest flag -8 exit after at least one accepted step.  A pair of decision_cases.UNREACHED
that an option set reaches is dropped from that list.

--part edges prints decision_cases.EDGES: the max_iter and acc_iters edge witnesses, derived by rule from the committed
cases (no search).
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
# (mode, scale, option overrides, option set: "" = the defaults)
MODES = [("cold", 0.0, {}, ""), ("cold", 0.0, {"mu0": 1e-2}, ""), ("warm", 0.0, {}, ""), ("disturbed", 0.1, {}, ""), ("disturbed", 0.3, {}, "")]
MODES += [(mode, scale, opts, oset) for oset, opts in dc.OPTION_SETS.items()
          for mode, scale in (("cold", 0.0), ("warm", 0.0), ("disturbed", 0.1), ("disturbed", 0.3))]
OPTION_GROUPS = ("", "+dense", "+N40")    # the groups the option sets are searched in (a witness each)


def branch_names(oset):
    if oset == "":
        return dc.DEFAULT_ONLY
    if oset == "ACC_OFF":
        return ["flag1"]
    return [k for k, sets in dc.OPTION_BRANCHES.items() if oset in sets]


def scan(job):
    """One loop: [(class, group, branch, option set, passes, Case)] of every solve that takes a branch, and the instances solved."""
    from oracle.oracle import Oracle
    from robot_mpcs_amd.scenarios import make_scenario
    cls, group, name, kw, seed, (mode, scale, opts, oset) = job
    steps = 1 if mode == "cold" else STEPS
    c = dc.Case(cls, name, kw, opts, seed, B, steps, mode, scale, 0, ())
    sc = dc.scenario_of(make_scenario, c)
    o = Oracle(sc.desc)
    o_def = dc.default_oracle(Oracle, sc, c) if dc.is_loose(opts) else None
    loop = dc.oracle_loop(sc, o, c)
    names = branch_names(oset)
    found = []
    for t, step in enumerate(loop):
        if mode != "cold" and t == 0:
            continue   # (the first step of a loop is the cold solve)
        cpu = step["cpu"]
        for b in range(B):
            if cpu["passes"][b] > dc.MAX_PASSES:
                continue
            view = dc.census_view(o, sc, c, step, b, o_def)
            took = tuple(k for k in names if dc.BRANCHES[k](view))
            cand = c._replace(steps=t + 1, witness=b, branches=took)
            for k in took:
                found.append((cls, group, k, oset, int(cpu["passes"][b]), cand))
                if oset and k == "flag2" and mode == "cold":    # (what the max_iter edge of decision_cases.EDGES needs)
                    found.append((cls, group, k, oset + " cold", int(cpu["passes"][b]), cand))
                if oset and k == "flag-8" and cpu["iters"][b] >= 1:    # (after accepted steps: the iterate has moved)
                    found.append((cls, group, k, oset + " later", int(cpu["passes"][b]), cand))
    return found, B * len(loop)


def _k(cand):
    return (dc.case_id(cand), cand.steps)


def robust(cand):
    from oracle.oracle import Oracle
    from robot_mpcs_amd.scenarios import make_scenario
    sc = dc.scenario_of(make_scenario, cand)
    o = Oracle(sc.desc)
    loop = dc.oracle_loop(sc, o, cand)
    ok = dc.rounding_insensitive(o, sc, cand, loop[-1])
    if ok and dc.is_loose(cand.opts):    # (the comparison solve at the default tolerances too)
        ok = dc.rounding_insensitive(dc.default_oracle(Oracle, sc, cand), sc, cand, loop[-1])
    return ok


def case_line(cand, branches, note):
    return "    Case(%r, %r, %r, %r, %d, %d, %d, %r, %r, %d, %r),   # %s" % (
        cand.cls, cand.name, cand.kw, cand.opts, cand.seed, cand.B, cand.steps, cand.mode, cand.scale, cand.witness,
        tuple(sorted(branches)), note)


def search(a, part):
    modes = [m for m in MODES if (m[3] == "") == (part == "default")]
    seeds = a.seeds if part == "default" else a.opt_seeds
    jobs = [(cls, g, n, kw, seed, m) for cls, g, n, kw in SCENARIOS for seed in range(1, seeds + 1) for m in modes
            if part == "default" or g in OPTION_GROUPS]
    with mp.Pool(a.jobs) as pool:
        res = pool.map(scan, jobs, chunksize=1)
        searched, cands = {}, {}
        for (found, n), job in zip(res, jobs):
            searched[(job[0], job[1])] = searched.get((job[0], job[1]), 0) + n
            for cls, g, k, oset, p, cand in found:
                cands.setdefault((cls, g, k, oset), []).append((p, cand))
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
    print("# cheapest rounding-insensitive witnesses per (class, group, branch, option set): passes, case")
    for key in sorted(kept):
        for p, cand in kept[key]:
            print("#   %-12s %-7s %-14s %-8s %3d  %s" % (key + (p, dc.case_id(cand))))
    return searched, cands, kept


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=12)
    ap.add_argument("--opt-seeds", type=int, default=4, help="seeds searched under the option sets")
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("--keep", type=int, default=3, help="robust witnesses kept per (class, group, branch)")
    ap.add_argument("--part", default="all", choices=("all", "default", "options", "edges"))
    a = ap.parse_args()
    os.environ.setdefault("OMP_NUM_THREADS", "1")
    if a.part == "edges":
        return print_edges()
    # (pairs the committed option witnesses reach; the options part below finds them again when it runs)
    reached_by_options = {(c.cls, k) for c in dc.CASES if set(c.opts) - {"mu0"} for k in c.branches}
    if a.part in ("all", "options"):
        searched, cands, kept = search(a, "options")
        # per (class, group) and branch: the cheapest witness over the option sets that reach it
        print("CASES += [")
        for cls, g in sorted(searched):
            for k, sets in dc.OPTION_BRANCHES.items():
                best = sorted([(p, oset, cand) for oset in sets for p, cand in kept.get((cls, g, k, oset), [])],
                              key=lambda t: (t[0], t[2].steps, t[2].seed, t[1]))
                if best:
                    p, oset, cand = best[0]
                    reached_by_options.add((cls, k))
                    print(case_line(cand, (k,), "%d passes, %s%s" % (p, oset, " (%s)" % g if g else "")))
                else:
                    print("    # (%r, %r, %r): no witness in %d instances per mode" % (cls, g, k, searched[(cls, g)] // (4 * len(dc.OPTION_SETS))))
        # the max_iter edge wants a COLD solve that ends with flag 2: per class without one at the default options, the
        # cheapest cold one under the option sets
        for cls in dc.CLASSES:
            if any(c.cls == cls and c.mode == "cold" and "flag2" in c.branches and not (set(c.opts) - {"mu0"}) for c in dc.CASES):
                continue
            best = sorted([(p, oset, cand) for (c_, g, k, oset), lst in kept.items() if c_ == cls and oset.endswith(" cold")
                           for p, cand in lst], key=lambda t: (t[0], t[2].seed, t[1], t[2].name))
            if best:
                p, oset, cand = best[0]
                print(case_line(cand, ("flag2",), "%d passes, %s" % (p, oset)))
            else:
                print("    # (%r, 'flag2', cold): no witness" % cls)
        # the cheapest flag -8 exits are failures of the first line search, where the returned iterate is the input: per
        # class, also the cheapest one after at least one accepted step
        for cls in dc.CLASSES:
            best = sorted([(p, oset, cand) for (c_, g, k, oset), lst in kept.items() if c_ == cls and oset.endswith(" later")
                           for p, cand in lst], key=lambda t: (t[0], t[2].steps, t[2].seed, t[1], t[2].name))
            if best:
                p, oset, cand = best[0]
                print(case_line(cand, ("flag-8",), "%d passes, %s" % (p, oset)))
            else:
                print("    # (%r, 'flag-8', after an accepted step): no witness" % cls)
        print("]")
    if a.part in ("all", "default"):
        searched, cands, kept = search(a, "default")
        # a small cover: per (class, group), greedily the witness that takes most of the branches still open
        print("CASES = [")
        for cls, g in sorted(searched):
            want = {k for k in dc.DEFAULT_ONLY if (cls, k) not in dc.NOT_APPLICABLE and kept.get((cls, g, k, ""))}
            pool_ = {_k(cand): (p, cand) for k in want for p, cand in kept[(cls, g, k, "")]}
            while want:
                p, cand = max(pool_.values(), key=lambda pc: (len(want & set(pc[1].branches)), -pc[0]))
                print(case_line(cand, want & set(cand.branches), "%d passes%s" % (p, " (%s)" % g if g else "")))
                want -= set(cand.branches)
        print("]")
        print("UNREACHED = {")
        for cls in dc.CLASSES:
            n = sum(v for (c_, g), v in searched.items() if c_ == cls)
            for k in dc.DEFAULT_ONLY:
                if (cls, k) in dc.NOT_APPLICABLE or (cls, k) in reached_by_options:
                    continue
                if not any(kept.get((cls, g, k, "")) for (c_, g) in searched if c_ == cls):
                    print("    (%r, %r): %d,%s" % (cls, k, n, "" if any((cls, g, k, "") in cands for (c_, g) in searched if c_ == cls)
                                                   else "   # (never seen, rounding filter aside)"))
        print("}")


def print_edges():
    from oracle.oracle import Oracle
    from robot_mpcs_amd.scenarios import make_scenario
    print("EDGES = [")
    for e in dc.derive_edges(make_scenario, Oracle):
        print("    %r," % (e,))
    print("]")


if __name__ == "__main__":
    main()
