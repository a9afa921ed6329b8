"""The whole-horizon reductions of the kernels (rmpc_inst.hpp: wave_sum / wave_max / wave_min / wave_reduce_many) exchange
lane values by vector moves -- v_permlane32_swap / v_permlane16_swap for the levels 32 and 16, DPP row rotations and quad
permutations below -- where they used to go through the LDS crossbar (__shfl_xor).  The shuffle form stays in the source
as the reference: ``rmpc_debug_wave_reduce`` runs one wavefront over the caller's lane values through both forms, and
the two results must be equal BIT FOR BIT IN EVERY LANE (NaN results: NaN in the same lanes, payloads not compared) --
for 32 and 64 lanes per instance, for the single reductions and for the two arities the kernels reduce together."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OPS = ("sum", "max", "min", "many541", "many102")
WORDS = {"sum": 1, "max": 1, "min": 1, "many541": 10, "many102": 3}


@pytest.fixture(scope="module")
def reduce_():
    import __graft_entry__ as g
    g.build()
    from robot_mpcs_amd._lib import debug_wave_reduce
    return debug_wave_reduce


def _same_bits(ref, new):
    nan = np.isnan(ref)
    assert np.array_equal(nan, np.isnan(new)), "NaN results in other lanes"
    a, b = ref.view(np.uint64), new.view(np.uint64)
    bad = np.argwhere((a != b) & ~nan)
    assert bad.size == 0, ("(word, lane) that differ", bad[:8], ref[tuple(bad[0])], new[tuple(bad[0])])


def _numpy_tree(v, lpi, fn):
    """the xor tree on the host: levels lpi / 2 .. 1, the lane's own value as first operand"""
    v = v.copy()
    lanes = np.arange(64)
    off = lpi // 2
    while off >= 1:
        v = fn(v, v[lanes ^ off])
        off //= 2
    return v


def _cases():
    rng = np.random.default_rng(2024)
    out = {}
    # sixteen decades, both signs
    out["decades"] = rng.standard_normal((10, 64)) * 10.0 ** rng.uniform(-8, 8, (10, 64))
    # denormals, mixed with zeros and the smallest normal numbers
    den = rng.integers(1, 1 << 52, (10, 64)).astype(np.uint64).view(np.float64) * rng.choice([-1.0, 1.0], (10, 64))
    den[rng.random((10, 64)) < 0.2] = 0.0
    den[rng.random((10, 64)) < 0.1] = np.finfo(np.float64).tiny
    out["denormals"] = den
    # infinities of both signs among ordinary numbers (sums of both give NaN: the same lanes in both forms)
    inf = rng.standard_normal((10, 64))
    inf[rng.random((10, 64)) < 0.05] = np.inf
    inf[rng.random((10, 64)) < 0.05] = -np.inf
    out["inf"] = inf
    pinf = rng.standard_normal((10, 64))
    pinf[:, 37] = np.inf
    pinf[5:, 3] = -np.inf
    out["one_inf"] = pinf
    out["all_equal"] = np.full((10, 64), 0.1) * np.arange(1, 11)[:, None]
    # signed zeros: alone, and among a few non-zero lanes
    z = np.where(rng.random((10, 64)) < 0.5, 0.0, -0.0)
    out["zeros"] = z
    zz = z.copy()
    zz[:, rng.integers(0, 64, 6)] = rng.standard_normal(6)
    out["zeros_mixed"] = zz
    out["all_minus_zero"] = np.full((10, 64), -0.0)
    # NaN inputs in some lanes
    nn = rng.standard_normal((10, 64))
    nn[rng.random((10, 64)) < 0.04] = np.nan
    out["nan"] = nn
    one = rng.standard_normal((10, 64))
    one[:, 21] = np.nan
    out["one_nan"] = one
    return out


CASES = _cases()


@pytest.mark.parametrize("lpi", [32, 64])
@pytest.mark.parametrize("op", OPS)
def test_vector_move_form_equals_shuffle_tree(reduce_, op, lpi):
    for name, v in CASES.items():
        ref, new = reduce_(v[:WORDS[op]], op, lpi)
        try:
            _same_bits(ref, new)
        except AssertionError as e:
            raise AssertionError((name,) + e.args) from None
        assert np.all(ref[WORDS[op] + (1 if op == "many102" else 0):] == 0.0)


@pytest.mark.parametrize("lpi", [32, 64])
def test_a_single_lane_reaches_every_lane_of_its_instance(reduce_, lpi):
    """One non-zero lane at each of the 64 positions: its value -- a different one per position and word -- arrives in
    exactly the lpi lanes of its instance and nowhere else (every lane's contribution and the rows the swap instructions
    pair), in both forms; the other instance keeps the neutral result."""
    lanes = np.arange(64)
    for pos in range(64):
        mine = (lanes // lpi) == (pos // lpi)
        for op in OPS:
            w = WORDS[op]
            val = 1.5 + pos + 0.25 * np.arange(w)
            if op in ("sum", "max"):
                v = np.zeros((w, 64))
            elif op == "min":
                v = np.full((w, 64), 1e300)
                val = -val
            elif op == "many541":
                v = np.zeros((w, 64)); v[9] = 1e300
            else:
                v = np.zeros((w, 64)); v[1:] = 1.0
                val = val.copy(); val[1:] = 1.0 / val[1:]
            rest = v[:, 0].copy()
            v[:, pos] = val
            ref, new = reduce_(v, op, lpi)
            _same_bits(ref, new)
            want = np.where(mine[None, :], val[:, None], rest[:, None])
            assert np.array_equal(new[:w], want), (op, pos)


@pytest.mark.parametrize("lpi", [32, 64])
def test_both_forms_are_the_xor_tree(reduce_, lpi):
    """The device trees against the same tree written in numpy (IEEE addition, maximum and minimum of finite numbers are
    the same operations on both sides): the reference form is what this file says it is."""
    v = CASES["decades"]
    for op, fn in (("sum", np.add), ("max", np.maximum), ("min", np.minimum)):
        ref, new = reduce_(v[:1], op, lpi)
        want = _numpy_tree(v[0], lpi, fn)
        assert np.array_equal(ref[0], want) and np.array_equal(new[0], want), op
    ref, new = reduce_(v, "many541", lpi)
    for w in range(10):
        fn = np.add if w < 5 else (np.maximum if w < 9 else np.minimum)
        want = _numpy_tree(v[w], lpi, fn)
        assert np.array_equal(ref[w], want) and np.array_equal(new[w], want), w
