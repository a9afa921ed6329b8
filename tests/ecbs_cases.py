"""The cases the focal search's test modules share (tests/test_ecbs_cpu.py asserts the outcome of every one,
tests/test_gpu_ecbs.py holds the device to ``ecbs_ref`` on them): the cases of tests/cbs_cases.py crossed with the
weights 1, 21/20, 3/2 and 2 -- ``CASES["<name>@<w_num>_<w_den>"]`` is the case's dict with ``w`` and ``want``, the outcome
the restatement must reach -- and the two store problems with the budgets their searches need."""
from cbs_cases import BUDGET, CASES as CBS_CASES, random_case
from cbs_reference import POOL, ROUNDS, SOLVED

WEIGHTS = ((1, 1), (21, 20), (3, 2), (2, 1))

# the budget cases end as they do under rmpc_cbs_device at the two small weights (the pool of 20 ids and the 7 rounds run
# out); at 3/2 and 2 the search is through after two expansions
_BUDGET_WANT = {"pool": {(1, 1): POOL, (21, 20): POOL}, "rounds": {(1, 1): ROUNDS, (21, 20): ROUNDS}}


def key(name, w):
    return "%s@%d_%d" % (name, w[0], w[1])


CASES = {key(name, w): dict(c, w=w, want=_BUDGET_WANT[name].get(w, SOLVED) if name in BUDGET else c["want"], base=name)
         for name, c in CBS_CASES.items() for w in WEIGHTS}

# The store of ``timed_reference.store_case`` (41 x 41, sep2 9, lag 1, four moves) at T 128, one node per round.  The
# budgets are taken from ``ecbs_ref`` on the CPU, once: with four robots, seed 0, at 21/20 it is through after 9
# expansions (cost 178, bound 173; SOLVED is seen in the round behind the last expansion), with sixteen at 11/10 after
# 351 (cost 696, bound 633, 702 nodes created).  Rounds and nodes leave a margin above that.
STORE = dict(T=128, sep2=9, lag=1, movement=4, expand=1)
STORE4 = dict(STORE, B=4, seed=0, w=(21, 20), rounds=16, nodes=64, expansions=9)
STORE16 = dict(STORE, B=16, seed=0, w=(11, 10), rounds=400, nodes=1024, expansions=351)

# A search with many nodes: four robots with sep2 4 on a 5 x 7 map, 64 nodes per round at weight 1.  The restatement
# creates 1767 nodes in 38 rounds, so a thread of k_ecbs_select sees up to eight ids, and three of its selections need a
# second pass (``repasses`` of ``ecbs_ref``).
MANY = dict(random_case(3, 5, 7, 4, 12, 4, 1, 4, density=0.1, nodes=4096, expand=64), w=(1, 1))
