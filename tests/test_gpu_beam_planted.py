"""The beamformed channel (Tracer.beam_channel) record by record, on planted workspaces (tests/planted.py): after a
real trace the test writes the records itself, so the reference sums values it chose.

  planted sums  against hermespy_rt_amd.beams.apply on the float64 array channel of the planted terms, for every part
                (LoS + scatter, LoS, scatter), with the negative controls of tests/test_gpu_pathsum_planted.py: the
                check also runs against a reference changed in one record (dropped, doubled, moved to the other
                polarisation) and must then fail.
  poison        every slot the kernels must not read is overwritten with NaN, then 1e30; the output stays bit-identical.

Bound: the UNIT_TOL = 0.05 of test_array_channel_against_float64 per element pair (a tenth of the weakest planted term),
times ||W_rx[a]||_1 ||W_tx[b]||_1 by the triangle inequality over the pairs.  Beam 0 of either codebook has a single
non-zero weight, so |g_rx[0] g_tx[0]| = ||W_rx[0]||_1 ||W_tx[0]||_1 for every direction: one record changes beam pair
(0, 0) by ten times its bound, whatever the other beams' patterns do to it."""
import numpy as np
import pytest

from hermespy_rt_amd import beams

from . import beam_util as BU
from . import planted as PL
from .beam_util import check_unit as _check
from .beam_util import planted_codebooks as _codebooks
from .pathsum_util import PARTS, _bits, _expect_failure, _force_los_classes, _traced

pytestmark = pytest.mark.gpu


def _sel(T, los, scatter):
    return PL.select(T, (T["los"] & los) | (~T["los"] & scatter))


@pytest.fixture(scope="module", params=["C3", "room"])
def planted(request, tmp_path_factory):
    tr, c = _traced(request.param, tmp_path_factory)
    T = PL.plant(tr)
    assert not PL.design_errors(T), PL.design_errors(T)
    yield request.param, tr, T
    tr.close()


@pytest.mark.parametrize("elements", ["2x3", "4x1"])
def test_beam_channel_against_float64(planted, elements):
    name, tr, T = planted
    lam = PL.C0 / (tr.f_ghz * 1e9)
    if elements == "2x3":
        rxe = np.array([[0, 0, 0], [0, lam / 2, 0]], np.float32)
        txe = np.array([[0, 0, 0], [lam / 2, 0, lam / 3], [0, lam / 4, lam / 2]], np.float32)
    else:
        rxe = (np.arange(4)[:, None] * np.array([[lam / 2, 0.0, 0.0]])).astype(np.float32)
        txe = np.zeros((1, 3), np.float32)
    wr, wt = _codebooks(rxe.shape[0], txe.shape[0])
    fa = tr.f_ghz * 1e9
    nk, nt, df = 16, 2, PL.FS / 4096
    f, t = PL.FC + np.arange(nk) * df, np.arange(nt) * PL.DT

    def ref(U):
        return beams.apply(PL.array_direct(U, tr.nrx, tr.ntx, rxe, txe, fa, f, t), wr, wt)

    full = None
    for los, scatter in PARTS:
        got = tr.beam_channel(rxe, txe, wr, wt, PL.FC, df, nk, 0.0, PL.DT, nt, los=los, scatter=scatter).cpu().numpy()
        worst = _check(got, ref(_sel(T, los, scatter)), wr, wt, "%s %s %s" % (name, elements, (los, scatter)))
        print(name, "beam", elements, (los, scatter), "max |err| / bound", worst)
        full = got if los and scatter else full
    _expect_failure(lambda U: _check(full, ref(U), wr, wt, "beam"), T, "beam " + elements)


def _run(tr, c, los, scatter):
    f0 = c["f_ghz"] * 1e9 - 32 * 30e3
    rxe = np.array([[0, 0, 0], [0, 0.04, 0]], np.float32)
    txe = np.array([[0, 0, 0], [0.04, 0, 0], [0, 0, 0.04]], np.float32)
    wr, wt = _codebooks(2, 3)
    out = _bits(tr.beam_channel(rxe, txe, wr, wt, f0, 30e3, 16, 1e-3, 2e-4, 2, los=los, scatter=scatter))
    tr.torch.cuda.synchronize(tr.device)
    return out


@pytest.mark.parametrize("name", ["C3", "room"])
def test_poison_does_not_change_the_output(name, tmp_path_factory):
    tr, c = _traced(name, tmp_path_factory)
    counts = tr.counts()
    _force_los_classes(tr)
    base = {parts: _run(tr, c, *parts) for parts in PARTS}
    for parts, b in base.items():
        assert bool(tr.torch.isfinite(b.view(tr.torch.float32)).all()), (name, parts)
    for value in (float("nan"), 1e30):
        hit = PL.poison(tr, counts, value)
        for cls in ("blocked_records", "tail_slots", "tail_mask_bits"):
            assert hit[cls] > 0, (name, cls, hit)
        if tr.nrx * tr.ntx > 1:
            assert hit["los_blocked"] > 0 and hit["los_coincident"] > 0, (name, hit)
        else:
            assert hit["los_blocked"] + hit["los_coincident"] > 0, (name, hit)
        for parts in PARTS:
            assert bool(tr.torch.equal(_run(tr, c, *parts), base[parts])), \
                "%s: beam channel with %s changed after poison %r" % (name, parts, value)
    tr.close()
