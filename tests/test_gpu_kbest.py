"""The K-best tree-search detection on planted tensors (Tracer.kbest -> hrt_channel_kbest; csrc/hrt_kbest.hip), no trace:
the exact plantings at tolerance 0 (device == rounded float64 reference == float32 emulation), the pruned
maximum-likelihood hypothesis, the standard-normal cases against the emulation to the bit at every point and under the
derived bounds at the points that are not fragile, the shapes Tracer.detect accepts too, the buffer rules, independence
of a point from its neighbours, determinism, non-finite points and null columns.  Outputs are pre-filled with NaN bytes
between guard bytes.  The cases and their design: tests/kbest_util.py, tests/test_kbest_design.py."""
import numpy as np
import pytest

from hermespy_rt_amd import abi
from hermespy_rt_amd import detect as DT

from . import configs as K
from . import kbest_util as U
from .pathsum_util import _tracer

pytestmark = pytest.mark.gpu

GUARD = 256


@pytest.fixture(scope="module")
def tr():
    t = _tracer(K.small(K.C1, 64))   # the detection reads only its tensors: nothing is traced
    yield t
    t.close()


def _run(tr, H, Y, S, noise, k, clip, srt=True, llr=True):
    """hrt_channel_kbest on the numpy tensors into NaN bytes between guards -> views of the numpy copy; the inputs are
    checked to be unchanged to the byte, the absent region to be absent"""
    torch = tr.torch
    nrx, ntx, nr, nt, _, T, K_ = H.shape
    B = S.shape[0].bit_length() - 1
    spec = abi.kbest_spec(nrx, ntx, nr, nt, T, K_, B, noise, k, clip, srt, llr)
    need = abi.kbest_regions(spec)[4]
    assert need == U.out_bytes(nrx, ntx, nt, B, T, K_, int(spec.flags))
    host_in = [np.array(a, np.complex64) for a in (H, Y, S)]
    d_H, d_Y, d_S = (torch.from_numpy(a).to(tr.device) for a in host_in)
    big = torch.full((need + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=tr.device)
    big[GUARD:GUARD + need] = 0xFF
    r = tr.kbest(d_H, d_Y, d_S, noise, k, clip, srt, llr, out=big[GUARD:GUARD + need])
    assert r["buffer"].data_ptr() == big.data_ptr() + GUARD
    torch.cuda.synchronize(tr.device)
    host = big.cpu().numpy()
    assert (host[:GUARD] == 0xA5).all() and (host[GUARD + need:] == 0xA5).all(), "written beyond the buffer"
    for d, a, name in zip((d_H, d_Y, d_S), host_in, ("H", "Y", "the constellation")):
        assert d.cpu().numpy().tobytes() == a.tobytes(), name + " was written"
    v = abi.kbest_views(host[GUARD:GUARD + need], spec)
    assert (v["llr"] is None) == (not llr)
    # every byte written: no NaN pattern is left (a non-finite point's index is all ones by definition)
    assert (v["status"] <= 2).all() and not np.isnan(v["metric"]).any()
    assert (v["index"][v["status"] != 1].astype(np.int64) < 1 << (nt * B)).all()
    assert (v["index"][v["status"] == 1] == U.NO_INDEX).all()
    if llr:
        assert not np.isnan(v["llr"]).any() and (np.abs(v["llr"]) <= np.float32(clip)).all()
    return v


# ---------------------------------------------------------------- tolerance 0

@pytest.mark.parametrize("case", U.PLANTINGS, ids=lambda c: c[0])
def test_plantings_at_tolerance_zero(tr, case):
    name, links, nr, nt, B, T, K_, k, srt, kind, n0, clip, emax, amp, special = case
    H, Y, S, _ = U.planting(case)
    dev = _run(tr, H, Y, S, n0, k, clip, srt)
    assert U.same(dev, U.rounded(U.reference(H, Y, S, n0, k, clip, srt))) is None
    assert U.same(dev, U.emulate(H, Y, S, n0, k, clip, srt)) is None
    assert (dev["status"] == (U.DEFICIENT if special == "null" or nr < nt else 0)).all()


def test_the_pruned_ml_hypothesis_stays_pruned(tr):
    H, Y, S, n0, clip, k, srt = U.pruned_case()
    dev = _run(tr, H, Y, S, n0, k, clip, srt)
    assert U.same(dev, U.emulate(H, Y, S, n0, k, clip, srt)) is None
    ml = tr.detect(*(tr.torch.from_numpy(np.array(a, np.complex64)).to(tr.device) for a in (H, Y, S)), n0)
    ml_index = ml["index"].cpu().numpy().view(np.uint32)
    differs = dev["index"] != ml_index
    assert differs.any() and not differs.all()
    assert (dev["metric"][differs] > ml["metric"].cpu().numpy()[differs]).all()


def test_the_zero_channel(tr):
    S = DT.qam(2, normalised=False).astype(np.complex64)
    rng = np.random.default_rng(5)
    H = np.zeros((1, 1, 3, 2, 2, 1, 3), np.complex64)
    Y = U.gaussian_integers(rng, (1, 1, 3, 2, 1, 3), 3)
    for k in (1, 4, 16):
        dev = _run(tr, H, Y, S, 0.5, k, 8.0)
        assert not dev["index"].any() and (dev["status"] == U.DEFICIENT).all()
        assert U.same(dev, U.emulate(H, Y, S, 0.5, k, 8.0)) is None
        if k == 16:
            assert not dev["llr"].any() and not np.signbit(dev["llr"]).any()


# ---------------------------------------------------------------- the standard-normal cases under the derived bounds

@pytest.mark.parametrize("case", U.NORMAL_CASES, ids=lambda c: c[0])
def test_normal_cases_under_the_derived_bounds(tr, case):
    name, links, nr, nt, B, T, K_, k, srt = case
    H, Y, S, sent = U.normal_case(case)
    dev = _run(tr, H, Y, S, U.NOISE, k, U.CLIP, srt)
    ref = U.reference(H, Y, S, U.NOISE, k, U.CLIP, srt)
    us = U.scale(H, Y, S)
    ok = U.sturdy(ref, nr, nt, srt)
    metric, llr = U.errors(dev, ref, us, U.NOISE, ok)
    print("%s: metric %.4f (bound %.3f) llr %.4f (bound %.3f) fragile %.3f"
          % (name, metric, U.METRIC_BOUND, llr, U.LLR_BOUND, 1.0 - ok.mean()))
    assert not dev["status"].any()
    assert 1.0 - ok.mean() <= U.FRAGILE_CAP
    assert metric <= U.METRIC_BOUND and llr <= U.LLR_BOUND
    assert U.index_agrees(dev, ref, us, ok, nr, nt)
    # the device follows the emulation to the bit, at every point
    assert U.same(dev, U.emulate(H, Y, S, U.NOISE, k, U.CLIP, srt)) is None


def _both(tr, nr, nt, B, k, points, seed):
    """kbest and Tracer.detect on a standard-normal case both accept"""
    case = ("both-%d" % seed, (1, 1), nr, nt, B, 1, points // 2, k, True)
    H, Y, S, _ = U.normal_case(case)
    dev = _run(tr, H, Y, S, U.NOISE, k, U.CLIP)
    t = tr.torch
    ml = tr.detect(*(t.from_numpy(np.array(a, np.complex64)).to(tr.device) for a in (H, Y, S)), U.NOISE)
    ml = {"index": ml["index"].cpu().numpy().view(np.uint32), "llr": ml["llr"].cpu().numpy()}
    ref = DT.ml_reference(H, Y, S, U.NOISE, table=True)
    d = np.sort(ref["distances"], -1)
    clear = d[..., 1] - d[..., 0] > 2.0 * U.METRIC_BOUND * U.scale(H, Y, S)
    return H, Y, S, dev, ml, clear


def test_where_no_parent_is_pruned_the_index_is_detects(tr):
    # 2 x 64-QAM, K = 64: M^(Nt - 1) = K
    H, Y, S, dev, ml, clear = _both(tr, 4, 2, 6, 64, 48, 1)
    assert clear.mean() > 0.9 and np.array_equal(dev["index"][clear], ml["index"][clear])


def test_where_the_list_is_exhaustive_the_llrs_are_detects_clamped(tr):
    # 3 x QPSK, K = 64: M^Nt = K
    H, Y, S, dev, ml, clear = _both(tr, 3, 3, 2, 64, 48, 2)
    assert clear.mean() > 0.9 and np.array_equal(dev["index"][clear], ml["index"][clear])
    us = U.scale(H, Y, S)[:, :, None, None]
    want = np.clip(ml["llr"].astype(np.float64), -U.CLIP, U.CLIP)
    # (two float32 results, each within the LLR bound of its exact value; detect's bound is the larger)
    from .detect_util import LLR_BOUND as DETECT_LLR_BOUND
    err = (np.abs(dev["llr"] - want) * U.NOISE / us).max()
    print("llr against detect: %.4f (bound %.3f)" % (err, U.LLR_BOUND + DETECT_LLR_BOUND))
    assert err <= U.LLR_BOUND + DETECT_LLR_BOUND


# ---------------------------------------------------------------- the buffer rules

def test_with_and_without_llrs_the_same_bits(tr):
    for case in (U.NORMAL_CASES[0], U.NORMAL_CASES[3], U.NORMAL_CASES[5]):
        name, links, nr, nt, B, T, K_, k, srt = case
        H, Y, S, _ = U.normal_case(case)
        full = _run(tr, H, Y, S, U.NOISE, k, U.CLIP, srt)
        bare = _run(tr, H, Y, S, U.NOISE, k, U.CLIP, srt, llr=False)
        assert bare["llr"] is None and U.same(bare, full, ("index", "status", "metric")) is None
        assert bare["buffer"].size == 12 * full["index"].size
        assert full["buffer"].size == bare["buffer"].size + 4 * full["llr"].size


def test_two_calls_give_the_same_bytes(tr):
    for case in (U.NORMAL_CASES[1], U.NORMAL_CASES[4]):
        name, links, nr, nt, B, T, K_, k, srt = case
        H, Y, S, _ = U.normal_case(case)
        a = _run(tr, H, Y, S, U.NOISE, k, U.CLIP, srt)
        b = _run(tr, H, Y, S, U.NOISE, k, U.CLIP, srt)
        assert a["buffer"].tobytes() == b["buffer"].tobytes()


def test_a_point_does_not_depend_on_its_neighbours(tr):
    for case in (U.NORMAL_CASES[3], U.NORMAL_CASES[0], U.NORMAL_CASES[5]):      # narrow (4 and 16 lanes) and wide
        name, links, nr, nt, B, T, K_, k, srt = case
        H, Y, S, _ = U.normal_case(case)
        base = _run(tr, H, Y, S, U.NOISE, k, U.CLIP, srt)
        nrx, ntx = links
        # the points permuted: links, pols, times and frequencies shuffled
        rng = np.random.default_rng(11)
        pr, pt, pp, pm, pk = (rng.permutation(n) for n in (nrx, ntx, 2, T, K_))
        Hp = H[pr][:, pt][:, :, :, :, pp][:, :, :, :, :, pm][..., pk]
        Yp = Y[pr][:, pt][:, :, :, pp][:, :, :, :, pm][..., pk]
        got = _run(tr, Hp, Yp, S, U.NOISE, k, U.CLIP, srt)
        for key in ("index", "status", "metric"):
            assert np.array_equal(got[key], base[key][pr][:, pt][:, :, pp][:, :, :, pm][..., pk]), key
        assert np.array_equal(got["llr"], base["llr"][pr][:, pt][:, :, :, :, pp][:, :, :, :, :, pm][..., pk])
        # one point alone, and every other point replaced
        alone = _run(tr, H[:1, :1, :, :, :, :1, :1], Y[:1, :1, :, :, :1, :1], S, U.NOISE, k, U.CLIP, srt)
        for key in ("index", "status", "metric"):
            assert np.array_equal(alone[key], base[key][:1, :1, :, :1, :1]), key
        assert np.array_equal(alone["llr"], base["llr"][:1, :1, :, :, :, :1, :1])
        H2, Y2 = U.normal(rng, H.shape), U.normal(rng, Y.shape)
        H2[0, 0, :, :, 1, 0, 0], Y2[0, 0, :, 1, 0, 0] = H[0, 0, :, :, 1, 0, 0], Y[0, 0, :, 1, 0, 0]
        other = _run(tr, H2, Y2, S, U.NOISE, k, U.CLIP, srt)
        for key in ("index", "status", "metric"):
            assert other[key][0, 0, 1, 0, 0] == base[key][0, 0, 1, 0, 0], key
        assert np.array_equal(other["llr"][0, 0, :, :, 1, 0, 0], base["llr"][0, 0, :, :, 1, 0, 0])


# ---------------------------------------------------------------- non-finite points and null columns

@pytest.mark.parametrize("where", ("H", "Y"))
@pytest.mark.parametrize("value", (np.nan, np.inf, 1e30), ids=("nan", "inf", "square-overflows"))
def test_non_finite_entries_flag_exactly_their_point(tr, value, where):
    for case in (U.NORMAL_CASES[0], U.NORMAL_CASES[5]):                        # narrow and wide
        name, links, nr, nt, B, T, K_, k, srt = case
        H, Y, S, _ = U.normal_case(case)
        clean = _run(tr, H, Y, S, U.NOISE, k, U.CLIP, srt)
        Hb, Yb = H.copy(), Y.copy()
        m, kk = H.shape[5] - 1, H.shape[6] - 2
        if where == "H":
            Hb[0, 0, 1, 0, 1, m, kk] = value
        else:
            Yb[0, 0, 1, 1, m, kk] = value
        dev = _run(tr, Hb, Yb, S, U.NOISE, k, U.CLIP, srt)
        flagged = np.zeros(dev["status"].shape, bool)
        flagged[0, 0, 1, m, kk] = True
        assert np.array_equal(dev["status"], np.where(flagged, U.NONFINITE, 0))
        assert (dev["index"][flagged] == U.NO_INDEX).all() and not dev["metric"][flagged].any()
        assert not dev["llr"][0, 0, :, :, 1, m, kk].any()
        # the neighbours come out bit-equal to the clean run
        for key in ("index", "metric"):
            assert np.array_equal(dev[key][~flagged], clean[key][~flagged]), key
        keep = np.broadcast_to(~flagged[:, :, None, None], dev["llr"].shape)
        assert np.array_equal(dev["llr"][keep], clean["llr"][keep])
        assert U.same(dev, U.emulate(Hb, Yb, S, U.NOISE, k, U.CLIP, srt)) is None
        assert U.same(_run(tr, Hb, Yb, S, U.NOISE, k, U.CLIP, srt, llr=False), dev,
                      ("index", "status", "metric")) is None


def test_an_llr_beyond_float_flags_the_point_only_with_llrs(tr):
    name, links, nr, nt, B, T, K_, k, srt = U.NORMAL_CASES[0]
    H, Y, S, _ = U.normal_case(U.NORMAL_CASES[0])
    n0 = 2.0 ** -140                    # (a float32 denormal: every quotient of a difference above 2^-12 overflows)
    dev = _run(tr, H, Y, S, n0, k, U.CLIP, srt)
    assert dev["status"].any()
    assert U.same(dev, U.emulate(H, Y, S, n0, k, U.CLIP, srt)) is None
    bare = _run(tr, H, Y, S, n0, k, U.CLIP, srt, llr=False)
    assert not bare["status"].any() and U.same(bare, U.emulate(H, Y, S, n0, k, U.CLIP, srt, llr=False)) is None


def test_null_columns_set_the_deficient_bit_only(tr):
    # a rank-one channel (every column a multiple of the first, exactly) and Nr < Nt, among regular points
    name, links, nr, nt, B, T, K_, k, srt = U.NORMAL_CASES[0]
    H, Y, S, _ = U.normal_case(U.NORMAL_CASES[0])
    H = H.copy()
    H[0, 0, :, :, 0, 0, 1] = H[0, 0, :, :1, 0, 0, 1] * np.array([1, 2, -1, 0.5], np.complex64)
    H[0, 0, :, 2, 1, 1, 3] = 0
    for s in (True, False):
        dev = _run(tr, H, Y, S, U.NOISE, k, U.CLIP, s)
        want = np.zeros(dev["status"].shape, np.uint32)
        want[0, 0, 0, 0, 1] = want[0, 0, 1, 1, 3] = U.DEFICIENT
        assert np.array_equal(dev["status"], want)
        assert np.isfinite(dev["metric"]).all() and (dev["index"] < 1 << (nt * B)).all()
        assert U.same(dev, U.emulate(H, Y, S, U.NOISE, k, U.CLIP, s)) is None
    wide = _run(tr, H[:, :, :2], Y[:, :, :2], S, U.NOISE, k, U.CLIP, False)
    assert (wide["status"] == U.DEFICIENT).all()
    assert U.same(wide, U.emulate(H[:, :, :2], Y[:, :, :2], S, U.NOISE, k, U.CLIP, False)) is None
