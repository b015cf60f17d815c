"""The codebook selection on planted tensors (Tracer.codebook_select -> hrt_codebook_select; csrc/hrt_codebook.hip), no
trace: plantings whose every intermediate is exact at tolerance 0 over every axis value and tile edge, the
standard-normal case list under the derived bounds and against the float32 emulation to the bit, the buffer rules,
independence of a subband from its neighbours and from the entries behind the winner, determinism, non-finite
subbands.  Outputs are pre-filled with NaN bytes between guard bytes.  The cases and their design:
tests/codebook_util.py, tests/test_codebook_design.py."""
import numpy as np
import pytest

from hermespy_rt_amd import abi
from hermespy_rt_amd import codebook as CB

from . import codebook_util as U
from . import configs as K
from .pathsum_util import _tracer

pytestmark = pytest.mark.gpu

GUARD = 256


@pytest.fixture(scope="module")
def tr():
    t = _tracer(K.small(K.C1, 64))   # the selection reads only its tensors: nothing is traced
    yield t
    t.close()


def _run(tr, H, W, metric, noise=None, S=None, table=True, effective=True):
    """hrt_codebook_select on the numpy tensors into NaN bytes between guards -> views of the numpy copy; the inputs
    are checked to be unchanged to the byte, the absent regions to be absent"""
    torch = tr.torch
    nrx, ntx, nr, nt, _, T, K_ = H.shape
    spec = abi.codebook_spec(nrx, ntx, nr, nt, T, K_, W.shape[2], W.shape[0], metric, noise, S, table, effective)
    need = abi.codebook_regions(spec)[5]
    assert need == U.out_bytes(nrx, ntx, nr, T, K_, W.shape[2], W.shape[0], int(spec.subband), int(spec.flags))
    d_H = torch.from_numpy(np.array(H, np.complex64)).to(tr.device)
    d_W = torch.from_numpy(np.array(W, np.complex64)).to(tr.device)
    big = torch.full((need + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=tr.device)
    big[GUARD:GUARD + need] = 0xFF
    r = tr.codebook_select(d_H, d_W, U.METRIC_NAME[metric], noise, S, table, effective, out=big[GUARD:GUARD + need])
    assert r["buffer"].data_ptr() == big.data_ptr() + GUARD
    torch.cuda.synchronize(tr.device)
    host = big.cpu().numpy()
    assert (host[:GUARD] == 0xA5).all() and (host[GUARD + need:] == 0xA5).all(), "written beyond the buffer"
    assert d_H.cpu().numpy().tobytes() == np.array(H, np.complex64).tobytes(), "H was written"
    assert d_W.cpu().numpy().tobytes() == np.array(W, np.complex64).tobytes(), "the codebook was written"
    v = abi.codebook_views(host[GUARD:GUARD + need], spec)
    assert (v["table"] is None) == (not table) and (v["effective"] is None) == (not effective)
    # every byte written: no NaN pattern is left (a flagged subband's index is all ones by definition)
    assert (v["status"] <= 1).all() and not np.isnan(v["metric"]).any()
    assert (v["index"][v["status"] == 0] < W.shape[0]).all() and (v["index"][v["status"] != 0] == U.NO_INDEX).all()
    for k in ("table", "effective"):
        if v[k] is not None:
            assert not np.isnan(v[k].view(np.float32)).any(), k
    return v


def _keys(table=True, effective=True):
    return ("index", "status", "metric") + (("table",) if table else ()) + (("effective",) if effective else ())


# ---------------------------------------------------------------- tolerance 0

@pytest.mark.parametrize("case", U.INTEGER_CASES, ids=lambda c: c[0])
def test_gaussian_integer_plantings_at_tolerance_zero(tr, case):
    H, W, S = U.integer_case(case)
    dev = _run(tr, H, W, U.POWER, None, S)
    assert U.same(dev, U.emulate(H, W, U.POWER, None, S)) is None


def test_capacity_with_one_layer_at_tolerance_zero(tr):
    H, W, S, n0 = U.capacity_l1_case()
    dev = _run(tr, H, W, U.CAPACITY, n0, S)
    assert U.same(dev, U.rounded(CB.select_reference(H, W, "capacity", n0, S))) is None


@pytest.mark.parametrize("shape", ((1, 1, 1), (2, 4, 2), (3, 33, 3), (16, 63, 4), (16, 64, 4)),
                         ids=lambda s: "%dx%d-l%d" % s)
def test_one_hot_plantings_pin_every_index(tr, shape):
    H, W, want = U.one_hot_case(*shape)
    dev = _run(tr, H, W, U.POWER, None, 1)
    assert np.array_equal(dev["index"].ravel(), want)
    assert U.same(dev, U.emulate(H, W, U.POWER, None, 1)) is None


def test_planted_ties_and_the_zero_channel(tr):
    H, W, S, c = U.tie_case()
    for metric in (U.POWER, U.CAPACITY):
        dev = _run(tr, H, W, metric, 0.5, S)
        assert (dev["index"] == c).all()
        assert U.same(dev, U.emulate(H, W, metric, 0.5, S)) is None
        zero = _run(tr, np.zeros_like(H), W, metric, 0.5, S)
        assert not zero["index"].any() and not zero["status"].any() and not zero["metric"].any()
        assert not zero["table"].any() and not zero["effective"].any()


# ---------------------------------------------------------------- the standard-normal cases under the derived bounds

@pytest.mark.parametrize("metric", (U.POWER, U.CAPACITY), ids=lambda m: U.METRIC_NAME[m])
@pytest.mark.parametrize("case", U.NORMAL_CASES, ids=lambda c: c[0])
def test_normal_cases_under_the_derived_bounds(tr, case, metric):
    H, W, S = U.normal_case(case)
    nr, nt = case[2], case[3]
    dev = _run(tr, H, W, metric, U.NOISE, S)
    ref = CB.select_reference(H, W, U.METRIC_NAME[metric], U.NOISE, S)
    mu = U.mu_error(dev["table"], ref["table"], nr, nt)
    eff = U.eff_error(dev["effective"], ref, H, W, dev["index"])
    ok, second = U.index_check(dev["index"], ref, nr, nt)
    print("%s %s: mu %.3f (bound %.3f) effective %.3f (bound %.3f) second rule %.3f"
          % (case[0], U.METRIC_NAME[metric], mu, U.MU_BOUND, eff, U.EFF_BOUND, second))
    assert not dev["status"].any()
    assert mu <= U.MU_BOUND and eff <= U.EFF_BOUND
    assert ok and second <= 0.05
    best = np.take_along_axis(np.moveaxis(dev["table"], 2, -1), dev["index"].astype(np.int64)[..., None], -1)[..., 0]
    assert np.array_equal(dev["metric"], best)
    # the log2 restatement holds: the device follows the emulation to the bit
    assert U.same(dev, U.emulate(H, W, metric, U.NOISE, S)) is None


# ---------------------------------------------------------------- the buffer rules

def test_every_flag_combination_writes_its_regions_and_the_same_bits(tr):
    H, W, S = U.normal_case(U.NORMAL_CASES[2])
    full = _run(tr, H, W, U.CAPACITY, U.NOISE, S)
    for table in (False, True):
        for effective in (False, True):
            got = _run(tr, H, W, U.CAPACITY, U.NOISE, S, table, effective)
            assert U.same(got, full, _keys(table, effective)) is None


def test_two_calls_give_the_same_bytes(tr):
    H, W, S = U.normal_case(U.NORMAL_CASES[5])
    a = _run(tr, H, W, U.CAPACITY, U.NOISE, S)
    b = _run(tr, H, W, U.CAPACITY, U.NOISE, S)
    assert a["buffer"].tobytes() == b["buffer"].tobytes()


def test_a_subband_does_not_depend_on_its_neighbours_or_on_entries_behind_the_winner(tr):
    case = U.NORMAL_CASES[2]                    # 2 x 2 links, T = 3, K = 5, S = 2: 72 subbands, the last of each short
    H, W, S = U.normal_case(case)
    for metric in (U.POWER, U.CAPACITY):
        base = _run(tr, H, W, metric, U.NOISE, S)
        # the subbands permuted: links, pols and times shuffled as blocks, and the two full subbands swapped
        rng = np.random.default_rng(11)
        pr, pt, pp, pm = rng.permutation(2), rng.permutation(2), rng.permutation(2), rng.permutation(3)
        kperm = np.array([2, 3, 0, 1, 4])
        Hp = H[pr][:, pt][:, :, :, :, pp][:, :, :, :, :, pm][..., kperm]
        got = _run(tr, Hp, W, metric, U.NOISE, S)
        bperm = np.array([1, 0, 2])
        for k in ("index", "status", "metric"):
            assert np.array_equal(got[k], base[k][pr][:, pt][:, :, pp][:, :, :, pm][..., bperm]), k
        assert np.array_equal(got["table"], base["table"][pr][:, pt][:, :, :, pp][:, :, :, :, pm][..., bperm])
        assert np.array_equal(got["effective"],
                              base["effective"][pr][:, pt][:, :, :, :, pp][:, :, :, :, :, pm][..., kperm])
        # entries appended behind the winner: weaker copies, over a tile edge (16 + 60 entries)
        more = np.concatenate([W, 0.5 * W[rng.integers(0, W.shape[0], 60)]])
        got = _run(tr, H, more, metric, U.NOISE, S)
        assert U.same(got, base, ("index", "status", "metric", "effective")) is None
        assert np.array_equal(got["table"][:, :, :W.shape[0]], base["table"])


# ---------------------------------------------------------------- non-finite subbands

@pytest.mark.parametrize("value", (np.nan, np.inf, 1e30), ids=("nan", "inf", "square-overflows"))
def test_non_finite_entries_flag_exactly_their_subband(tr, value):
    H, W, S = U.normal_case(U.NORMAL_CASES[0])              # K = 24, S = 12: two subbands per pol
    Hb = H.copy()
    Hb[0, 0, 1, 2, 1, 0, S + 1] = value                     # planted in one frequency: pol 1, subband 1
    for metric in (U.POWER, U.CAPACITY):
        clean = _run(tr, H, W, metric, U.NOISE, S)
        dev = _run(tr, Hb, W, metric, U.NOISE, S)
        flagged = np.zeros(dev["status"].shape, bool)
        flagged[0, 0, 1, 0, 1] = True
        assert np.array_equal(dev["status"], np.where(flagged, U.NONFINITE, 0))
        assert (dev["index"][flagged] == U.NO_INDEX).all() and not dev["metric"][flagged].any()
        assert not dev["table"][0, 0, :, 1, 0, 1].any() and not dev["effective"][0, 0, :, :, 1, 0, S:].any()
        # the neighbours come out bit-equal to the clean run
        for k in ("index", "metric"):
            assert np.array_equal(dev[k][~flagged], clean[k][~flagged]), k
        assert np.array_equal(dev["table"][:, :, :, 0], clean["table"][:, :, :, 0])
        assert np.array_equal(dev["table"][0, 0, :, 1, 0, 0], clean["table"][0, 0, :, 1, 0, 0])
        assert np.array_equal(dev["effective"][:, :, :, :, 0], clean["effective"][:, :, :, :, 0])
        assert np.array_equal(dev["effective"][0, 0, :, :, 1, 0, :S], clean["effective"][0, 0, :, :, 1, 0, :S])
        assert U.same(dev, U.emulate(Hb, W, metric, U.NOISE, S)) is None
