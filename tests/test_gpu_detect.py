"""The maximum-likelihood detection on planted tensors (Tracer.detect -> hrt_channel_detect; csrc/hrt_detect.hip), no
trace: plantings whose every distance and LLR is exact at tolerance 0 over every switch of the form, planted ties
(within a tile and across a tile edge), one-hot plantings, the zero channel, the standard-normal case list under the
derived bounds and against the float32 emulation to the bit, the buffer rules, independence of a point from its
neighbours, determinism, non-finite points.  Outputs are pre-filled with NaN bytes between guard bytes.  The cases and
their design: tests/detect_util.py, tests/test_detect_design.py."""
import numpy as np
import pytest

from hermespy_rt_amd import abi
from hermespy_rt_amd import detect as DT

from . import configs as K
from . import detect_util as U
from .pathsum_util import _tracer

pytestmark = pytest.mark.gpu

GUARD = 256


@pytest.fixture(scope="module")
def tr():
    t = _tracer(K.small(K.C1, 64))   # the detection reads only its tensors: nothing is traced
    yield t
    t.close()


def _run(tr, H, Y, S, noise, llr=True):
    """hrt_channel_detect on the numpy tensors into NaN bytes between guards -> views of the numpy copy; the inputs are
    checked to be unchanged to the byte, the absent region to be absent"""
    torch = tr.torch
    nrx, ntx, nr, nt, _, T, K_ = H.shape
    B = S.shape[0].bit_length() - 1
    spec = abi.detect_spec(nrx, ntx, nr, nt, T, K_, B, noise, llr)
    need = abi.detect_regions(spec)[4]
    assert need == U.out_bytes(nrx, ntx, nt, B, T, K_, int(spec.flags))
    host_in = [np.array(a, np.complex64) for a in (H, Y, S)]
    d_H, d_Y, d_S = (torch.from_numpy(a).to(tr.device) for a in host_in)
    big = torch.full((need + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=tr.device)
    big[GUARD:GUARD + need] = 0xFF
    r = tr.detect(d_H, d_Y, d_S, noise, llr, out=big[GUARD:GUARD + need])
    assert r["buffer"].data_ptr() == big.data_ptr() + GUARD
    torch.cuda.synchronize(tr.device)
    host = big.cpu().numpy()
    assert (host[:GUARD] == 0xA5).all() and (host[GUARD + need:] == 0xA5).all(), "written beyond the buffer"
    for d, a, name in zip((d_H, d_Y, d_S), host_in, ("H", "Y", "the constellation")):
        assert d.cpu().numpy().tobytes() == a.tobytes(), name + " was written"
    v = abi.detect_views(host[GUARD:GUARD + need], spec)
    assert (v["llr"] is None) == (not llr)
    # every byte written: no NaN pattern is left (a flagged point's index is all ones by definition)
    assert (v["status"] <= 1).all() and not np.isnan(v["metric"]).any()
    assert (v["index"][v["status"] == 0] < 1 << (nt * B)).all() and (v["index"][v["status"] != 0] == U.NO_INDEX).all()
    if llr:
        assert not np.isnan(v["llr"]).any()
    return v


# ---------------------------------------------------------------- tolerance 0

@pytest.mark.parametrize("case", U.INTEGER_CASES, ids=lambda c: c[0])
def test_gaussian_integer_plantings_at_tolerance_zero(tr, case):
    H, Y, S, n0, _ = U.integer_case(case)
    dev = _run(tr, H, Y, S, n0)
    assert U.same(dev, U.rounded(DT.ml_reference(H, Y, S, n0))) is None
    assert U.same(dev, U.emulate(H, Y, S, n0)) is None


@pytest.mark.parametrize("shape", ((1, 1, 1), (2, 3, 2), (5, 2, 6), (3, 12, 1), (64, 1, 6), (2, 1, 8), (2, 4, 3)),
                         ids=lambda s: "%dx%d-b%d" % s)
def test_one_hot_plantings_pin_every_row_stream_and_bit(tr, shape):
    H, Y, S, want = U.one_hot_case(*shape)
    dev = _run(tr, H, Y, S, 1.0)
    assert np.array_equal(dev["index"].ravel(), want)
    assert U.same(dev, U.emulate(H, Y, S, 1.0)) is None


def test_planted_ties_within_a_tile_and_across_a_tile_edge(tr):
    for name, H, Y, S, n0, want, zero_bits in U.tie_cases():
        nt, B = H.shape[3], S.shape[0].bit_length() - 1
        dev = _run(tr, H, Y, S, n0)
        assert np.array_equal(dev["index"].ravel(), want), name
        L = np.moveaxis(dev["llr"], (2, 3), (-2, -1)).reshape(-1, nt, B)
        for j in range(nt):
            for b in range(B):
                if U.bit_position(B, j, b) in zero_bits:
                    assert not L[:, j, b].any() and not np.signbit(L[:, j, b]).any(), (name, j, b)
        assert U.same(dev, U.emulate(H, Y, S, n0)) is None, name


def test_the_zero_channel_ties_everywhere(tr):
    for nt, B in ((2, 2), (7, 1), (3, 4)):
        rng = np.random.default_rng(nt)
        S = DT.qam(B, normalised=False).astype(np.complex64)
        H = np.zeros((1, 1, 3, nt, 2, 1, 3), np.complex64)
        Y = U.gaussian_integers(rng, (1, 1, 3, 2, 1, 3), 3)
        dev = _run(tr, H, Y, S, 0.5)
        assert not dev["index"].any() and not dev["status"].any() and not dev["llr"].any()
        assert not np.signbit(dev["llr"]).any()
        assert U.same(dev, U.emulate(H, Y, S, 0.5)) is None


# ---------------------------------------------------------------- the standard-normal cases under the derived bounds

@pytest.mark.parametrize("case", U.NORMAL_CASES, ids=lambda c: c[0])
def test_normal_cases_under_the_derived_bounds(tr, case):
    H, Y, S, sent = U.normal_case(case)
    dev = _run(tr, H, Y, S, U.NOISE)
    ref = DT.ml_reference(H, Y, S, U.NOISE, table=True)
    us = U.scale(H, Y, S)
    metric = U.metric_error(dev["metric"], ref, us, dev["index"])
    llr = U.llr_error(dev["llr"], ref, us, U.NOISE)
    ok, second = U.index_check(dev["index"], ref, us)
    print("%s: metric %.3f (bound %.3f) llr %.3f (bound %.3f) second rule %.3f"
          % (case[0], metric, U.METRIC_BOUND, llr, U.LLR_BOUND, second))
    assert not dev["status"].any()
    assert metric <= U.METRIC_BOUND and llr <= U.LLR_BOUND
    assert ok and second <= 0.05
    # the signs of the LLRs are the bits of the hard decision
    bits = np.moveaxis(DT.hard_bits(dev["index"], case[3], case[4]), (-2, -1), (2, 3))
    assert ((dev["llr"] > 0) == (bits == 1))[dev["llr"] != 0].all()
    # the device follows the emulation to the bit
    assert U.same(dev, U.emulate(H, Y, S, U.NOISE)) is None


# ---------------------------------------------------------------- the buffer rules

def test_with_and_without_llrs_the_same_bits(tr):
    for case in (U.NORMAL_CASES[0], U.NORMAL_CASES[3], U.NORMAL_CASES[8]):
        H, Y, S, _ = U.normal_case(case)
        full = _run(tr, H, Y, S, U.NOISE)
        bare = _run(tr, H, Y, S, U.NOISE, llr=False)
        assert bare["llr"] is None and U.same(bare, full, ("index", "status", "metric")) is None
        assert bare["buffer"].size == 12 * full["index"].size
        assert full["buffer"].size == bare["buffer"].size + 4 * full["llr"].size


def test_two_calls_give_the_same_bytes(tr):
    for case in (U.NORMAL_CASES[1], U.NORMAL_CASES[4]):
        H, Y, S, _ = U.normal_case(case)
        a = _run(tr, H, Y, S, U.NOISE)
        b = _run(tr, H, Y, S, U.NOISE)
        assert a["buffer"].tobytes() == b["buffer"].tobytes()


def test_a_point_does_not_depend_on_its_neighbours(tr):
    for case in (U.NORMAL_CASES[5], U.NORMAL_CASES[0], U.NORMAL_CASES[1]):      # narrow (2 and 16 lanes) and wide
        H, Y, S, _ = U.normal_case(case)
        base = _run(tr, H, Y, S, U.NOISE)
        nrx, ntx, _, _, _, T, K_ = H.shape
        # the points permuted: links, pols, times and frequencies shuffled
        rng = np.random.default_rng(11)
        pr, pt, pp, pm, pk = (rng.permutation(n) for n in (nrx, ntx, 2, T, K_))
        Hp = H[pr][:, pt][:, :, :, :, pp][:, :, :, :, :, pm][..., pk]
        Yp = Y[pr][:, pt][:, :, :, pp][:, :, :, :, pm][..., pk]
        got = _run(tr, Hp, Yp, S, U.NOISE)
        for k in ("index", "status", "metric"):
            assert np.array_equal(got[k], base[k][pr][:, pt][:, :, pp][:, :, :, pm][..., pk]), k
        assert np.array_equal(got["llr"], base["llr"][pr][:, pt][:, :, :, :, pp][:, :, :, :, :, pm][..., pk])
        # one point alone, and every other point replaced
        alone = _run(tr, H[:1, :1, :, :, :, :1, :1], Y[:1, :1, :, :, :1, :1], S, U.NOISE)
        for k in ("index", "status", "metric"):
            assert np.array_equal(alone[k], base[k][:1, :1, :, :1, :1]), k
        assert np.array_equal(alone["llr"], base["llr"][:1, :1, :, :, :, :1, :1])
        H2, Y2 = U.normal(rng, H.shape), U.normal(rng, Y.shape)
        H2[0, 0, :, :, 1, 0, 0], Y2[0, 0, :, 1, 0, 0] = H[0, 0, :, :, 1, 0, 0], Y[0, 0, :, 1, 0, 0]
        other = _run(tr, H2, Y2, S, U.NOISE)
        for k in ("index", "status", "metric"):
            assert other[k][0, 0, 1, 0, 0] == base[k][0, 0, 1, 0, 0], k
        assert np.array_equal(other["llr"][0, 0, :, :, 1, 0, 0], base["llr"][0, 0, :, :, 1, 0, 0])


# ---------------------------------------------------------------- non-finite points

@pytest.mark.parametrize("where", ("H", "Y"))
@pytest.mark.parametrize("value", (np.nan, np.inf, 1e30), ids=("nan", "inf", "square-overflows"))
def test_non_finite_entries_flag_exactly_their_point(tr, value, where):
    for case in (U.NORMAL_CASES[0], U.NORMAL_CASES[1]):                        # narrow and wide
        H, Y, S, _ = U.normal_case(case)
        clean = _run(tr, H, Y, S, U.NOISE)
        Hb, Yb = H.copy(), Y.copy()
        m, k = H.shape[5] - 1, H.shape[6] - 2
        if where == "H":
            Hb[0, 0, 1, 0, 1, m, k] = value
        else:
            Yb[0, 0, 1, 1, m, k] = value
        dev = _run(tr, Hb, Yb, S, U.NOISE)
        flagged = np.zeros(dev["status"].shape, bool)
        flagged[0, 0, 1, m, k] = True
        assert np.array_equal(dev["status"], np.where(flagged, U.NONFINITE, 0))
        assert (dev["index"][flagged] == U.NO_INDEX).all() and not dev["metric"][flagged].any()
        assert not dev["llr"][0, 0, :, :, 1, m, k].any()
        # the neighbours come out bit-equal to the clean run
        for key in ("index", "metric"):
            assert np.array_equal(dev[key][~flagged], clean[key][~flagged]), key
        keep = np.broadcast_to(~flagged[:, :, None, None], dev["llr"].shape)
        assert np.array_equal(dev["llr"][keep], clean["llr"][keep])
        assert U.same(dev, U.emulate(Hb, Yb, S, U.NOISE)) is None
        assert U.same(_run(tr, Hb, Yb, S, U.NOISE, llr=False), dev, ("index", "status", "metric")) is None


def test_an_llr_beyond_float_flags_the_point_only_with_llrs(tr):
    H, Y, S, _ = U.normal_case(U.NORMAL_CASES[0])
    n0 = 2.0 ** -126
    dev = _run(tr, H, Y, S, n0)
    assert dev["status"].any()
    assert U.same(dev, U.emulate(H, Y, S, n0)) is None
    bare = _run(tr, H, Y, S, n0, llr=False)
    assert not bare["status"].any() and U.same(bare, U.emulate(H, Y, S, n0, llr=False)) is None
