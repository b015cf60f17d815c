"""Spatial covariance matrices on the device (Tracer.array_covariance, hermespy_rt.compute_array_covariance) on planted
workspaces (tests/planted.py, tests/covariance_util.py; the design is proven in tests/test_covariance_design.py).

  1. exact: on the exact planting every entry is a sum of multiples of 1/4 below 2^22, so R_rx (scatter and LoS) and
     the LoS part of R_tx equal the float64 reference at tolerance 0, for sizes around every tile and block edge.
  2. generic: both sides with traced directions and half-wavelength arrays against the float64 reference within
     CU.TOL = 1/32, an eighth of the smallest planted p, with every negative control (a record dropped, doubled or
     moved to the other polarisation; every wrong result of CU.MUTANTS) failing.
  3. against the coherent family: array_channel over a DFT grid of the planted delays, contracted on the host.
  4. against power_profiles: trace(R) = N P, and a single element at the origin gives P.
  5. chunks, parts, sides, accumulate, shards, a link without terms.   6. poison.   7. the drop-in entries.

Every output is also Hermitian to the bit with a real diagonal (CU.check).  The device's sincospif is exact at the
multiples of 1/2 the exact planting uses: item 1 holds at tolerance 0."""
import ctypes as C
import sys

import numpy as np
import pytest

from hermespy_rt_amd import abi
from hermespy_rt_amd import covariance as CV

from . import configs as K
from . import covariance_util as CU
from . import planted as PL
from .pathsum_util import PARTS, _bits, _expect_failure, _force_los_classes, _tracer

pytestmark = pytest.mark.gpu

ALL_PARTS = PARTS + ((False, False),)


def _np(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def _sel(T, los, scatter):
    return PL.select(T, (T["los"] & los) | (~T["los"] & scatter))


def _small():
    """C4_DOPPLER at 1100 rays: two record chunks, 2 x 2 links"""
    tr = _tracer(K.small(K.C4_DOPPLER, 1100))
    tr.trace()
    return tr


@pytest.fixture(scope="module")
def generic():
    """PL.plant with the traced directions"""
    tr = _small()
    T = PL.plant(tr)
    assert not PL.design_errors(T), PL.design_errors(T)
    yield tr, T
    tr.close()


@pytest.fixture(scope="module")
def exact():
    """the exact planting of tests/covariance_util.py"""
    tr = _small()
    T = CU.plant_exact(tr, PL.plant(tr))
    assert not PL.design_errors(T), PL.design_errors(T)
    assert set(range(6)) == set(CU.axis_of(T)[~T["los"]])
    yield tr, T
    tr.close()


def _half_wavelength(tr, elements):
    """the arrays of tests/test_gpu_pathsum_planted.py"""
    lam = PL.C0 / (tr.f_ghz * 1e9)
    if elements == "2x2":
        return (np.array([[0, 0, 0], [0, lam / 2, 0]], np.float32),
                np.array([[0, 0, 0], [lam / 2, 0, lam / 3]], np.float32))
    return (np.arange(4)[:, None] * np.array([[lam / 2, 0.0, 0.0]])).astype(np.float32), np.zeros((1, 3), np.float32)


def _nchunks(tr, nr, nt):
    """the record chunks of a call, from its scratch size (csrc/hrt_covariance.h: seg, then complex
    [link][side][chunk][pol][block][64][64])"""
    spec = abi.covariance_spec(nr > 0, nt > 0)
    a = abi.ArraySpec(nr, nt, 0x1000, 0x1000, CU.F_A)
    need = C.c_uint64(0)
    assert tr.L.hrt_array_covariance_scratch_bytes(tr.problem, C.byref(tr.shard), C.byref(spec), C.byref(a),
                                                   C.byref(need)) == 0
    seg = (tr.nb * (tr.ntx + 1) * 4 + 255) // 256 * 256
    blocks = sum(((n + 63) // 64) * ((n + 63) // 64 + 1) // 2 for n in (nr, nt))
    per = tr.nrx * tr.ntx * 2 * blocks * 64 * 64 * 8
    assert (need.value - seg) % per == 0
    return (need.value - seg) // per


# ------------------------------------------------------------------ 1. exact
@pytest.mark.parametrize("n", CU.SIZES)
def test_rx_covariance_is_exact_on_the_exact_planting(exact, n):
    tr, T = exact
    e = CU.exact_elements(n)
    got = _np(tr.array_covariance(rx_elements=e, array_frequency=CU.F_A))
    assert got["rx"].shape == (tr.nrx, tr.ntx, 2, n, n) and got["tx"].size == 0
    ref = CU.reference(T, tr.nrx, tr.ntx, e, CU.F_A, "rx")
    assert (np.abs(ref).reshape(tr.nrx * tr.ntx, -1).max(axis=1) >= 1).all()
    CU.check(got["rx"], ref, 0.0, "R_rx exact N = %d" % n, T, tr.ntx)
    if n in (17, 65):   # the negative controls at tolerance 0
        for name in CU.MUTANTS:
            with pytest.raises(AssertionError):
                CU.check(got["rx"], CU.mutant(name, T, tr.nrx, tr.ntx, e, CU.F_A, "rx"), 0.0, name)


@pytest.mark.parametrize("n", [1, 17, 33, 65])
def test_tx_covariance_of_the_los_part_is_exact(exact, n):
    tr, T = exact
    e = CU.exact_elements(n, salt=1)
    got = _np(tr.array_covariance(tx_elements=e, scatter=False, array_frequency=CU.F_A))
    assert got["tx"].shape == (tr.nrx, tr.ntx, 2, n, n) and got["rx"].size == 0
    Tl = _sel(T, True, False)
    assert Tl["rx"].size > 0 and (PL.los_status(tr) == 2).any()
    CU.check(got["tx"], CU.reference(Tl, tr.nrx, tr.ntx, e, CU.F_A, "tx"), 0.0, "R_tx LoS exact N = %d" % n)
    if n > 1:
        with pytest.raises(AssertionError):
            CU.check(got["tx"], CU.mutant("urx_utx_swapped", Tl, tr.nrx, tr.ntx, e, CU.F_A, "tx"), 0.0, "swapped")


# ------------------------------------------------------------------ 2. generic
def _check_both(got, T, tr, rxe, txe, fa, tol, what, ref=None):
    refs = ref or {s: CU.reference(T, tr.nrx, tr.ntx, e, fa, s) for s, e in (("rx", rxe), ("tx", txe))}
    return max(CU.check(got[s], refs[s], tol, "%s R_%s" % (what, s), T, tr.ntx) for s in ("rx", "tx"))


@pytest.mark.parametrize("elements", ["2x2", "4x1"])
def test_both_sides_against_float64(generic, elements):
    tr, T = generic
    rxe, txe = _half_wavelength(tr, elements)
    assert rxe.shape[0] != txe.shape[0] or elements == "2x2"
    fa = tr.f_ghz * 1e9
    # the measured f32-MFMA error (CU.F32_MFMA_ERR) leaves room below the tolerance
    assert (CU.F32_MFMA_ERR * CU.total_power(T, tr.nrx, tr.ntx) <= CU.TOL / 8).all()
    full = None
    for los, scatter in PARTS:
        got = _np(tr.array_covariance(rxe, txe, los=los, scatter=scatter))
        err = _check_both(got, _sel(T, los, scatter), tr, rxe, txe, fa, CU.TOL, "generic %s" % elements)
        print("covariance", elements, (los, scatter), "largest |error|", err)
        full = got if los and scatter else full
    _expect_failure(lambda U: _check_both(full, U, tr, rxe, txe, fa, CU.TOL, "control"), T, "covariance")
    for name in CU.MUTANTS:
        bad = {s: CU.mutant(name, T, tr.nrx, tr.ntx, e, fa, s) for s, e in (("rx", rxe), ("tx", txe))}
        with pytest.raises(AssertionError):
            _check_both(full, T, tr, rxe, txe, fa, CU.TOL, name, ref=bad)
            print("the check passed with the mutant", name)


# ------------------------------------------------------------------ 3. against the coherent family
def test_covariance_is_the_dft_contraction_of_array_channel(generic):
    tr, T = generic
    rxe, txe = _half_wavelength(tr, "2x2")
    nr, nt = rxe.shape[0], txe.shape[0]
    nk = 1 << int(np.ceil(np.log2(T["n"].max() + 1)))
    H = tr.array_channel(rxe, txe, PL.FC, PL.FS / nk, nk).cpu().numpy().astype(np.complex128)[..., 0, :]
    want_rx = np.einsum("rtijpk,rtljpk->rtpil", H, H.conj()) / (nk * nt)
    want_tx = np.einsum("rtijpk,rtilpk->rtpjl", H, H.conj()) / (nk * nr)
    got = _np(tr.array_covariance(rxe, txe))
    for side, want in (("rx", want_rx), ("tx", want_tx)):
        want = 0.5 * (want + want.conj().swapaxes(-1, -2))   # (the contraction is Hermitian up to float64 rounding)
        err = CU.check(got[side], want, CU.TOL, "DFT contraction R_" + side, T, tr.ntx)
        print("covariance against array_channel", side, "K", nk, "largest |error|", err)


# ------------------------------------------------------------------ 4. against power_profiles
def test_trace_and_single_element_against_power_profiles(exact):
    tr, T = exact
    for los, scatter in PARTS:
        P = tr.power_profiles(0.0, 1e-9, 0, los=los, scatter=scatter)["moments"][..., abi.POWER_P].cpu().numpy()
        e = CU.exact_elements(17)
        R = _np(tr.array_covariance(rx_elements=e, los=los, scatter=scatter, array_frequency=CU.F_A))["rx"]
        assert np.array_equal(np.trace(R, axis1=-2, axis2=-1), (17 * P).astype(np.complex64)), (los, scatter)
        one = _np(tr.array_covariance(np.zeros((1, 3)), np.zeros((1, 3)), los=los, scatter=scatter))
        assert np.array_equal(one["rx"][..., 0, 0], P.astype(np.complex64)), (los, scatter)
        assert np.array_equal(one["tx"][..., 0, 0], P.astype(np.complex64)), (los, scatter)


# ------------------------------------------------------------------ 5. chunks, parts, sides, accumulate, shards
@pytest.mark.parametrize("rays,chunks", [(600, "one"), (1100, "two"), (20000, "many")])
def test_record_chunks(rays, chunks):
    tr = _tracer(K.small(K.C4_DOPPLER, rays))
    tr.trace()
    n = _nchunks(tr, 33, 17)
    assert {"one": n == 1, "two": n == 2, "many": n > 2}[chunks], n
    T = CU.plant_exact(tr, PL.plant(tr))
    rxe, txe = CU.exact_elements(33), CU.exact_elements(17, salt=1)
    got = _np(tr.array_covariance(rxe, txe, array_frequency=CU.F_A))
    CU.check(got["rx"], CU.reference(T, tr.nrx, tr.ntx, rxe, CU.F_A, "rx"), 0.0, "R_rx %d rays" % rays, T, tr.ntx)
    # u_tx is traced: float32 sums of up to sum_p p, with the headroom of item 2 over the measured f32-MFMA error
    tol = max(CU.TOL, 8 * CU.F32_MFMA_ERR * CU.total_power(T, tr.nrx, tr.ntx).max())
    assert tol < 0.125, tol   # half the smallest planted p
    err = CU.check(got["tx"], CU.reference(T, tr.nrx, tr.ntx, txe, CU.F_A, "tx"), tol, "R_tx %d rays" % rays, T, tr.ntx)
    print("covariance", rays, "rays", n, "chunks: largest |error| of R_tx", err, "tolerance", tol)
    tr.close()


def test_parts_sides_and_accumulate(exact):
    tr, T = exact
    rxe, txe = CU.exact_elements(17), CU.exact_elements(5, salt=1)
    refs = {}
    for los, scatter in ALL_PARTS:
        if not (los or scatter):
            with pytest.raises(ValueError, match="parts"):
                tr.array_covariance(rxe, txe, los=los, scatter=scatter, array_frequency=CU.F_A)
            continue
        got = _np(tr.array_covariance(rxe, txe, los=los, scatter=scatter, array_frequency=CU.F_A))
        refs[los, scatter] = got
        CU.check(got["rx"], CU.reference(_sel(T, los, scatter), tr.nrx, tr.ntx, rxe, CU.F_A, "rx"), 0.0,
                 "R_rx parts %s" % ((los, scatter),), T, tr.ntx)
    both = refs[True, True]
    # the parts add up (exact sums on the RX side; the TX side within float32 rounding of the scatter part)
    assert np.array_equal(refs[True, False]["rx"] + refs[False, True]["rx"], both["rx"])
    assert np.abs(refs[True, False]["tx"] + refs[False, True]["tx"] - both["tx"]).max() <= CU.TOL
    # one side alone is that side of the call with both, bit for bit
    only_rx = _np(tr.array_covariance(rx_elements=rxe, array_frequency=CU.F_A))
    only_tx = _np(tr.array_covariance(tx_elements=txe, array_frequency=CU.F_A))
    assert np.array_equal(only_rx["rx"], both["rx"]) and only_rx["tx"].size == 0
    assert np.array_equal(only_tx["tx"], both["tx"]) and only_tx["rx"].size == 0
    with pytest.raises(ValueError, match="sides"):
        tr.array_covariance(array_frequency=CU.F_A)
    # two calls give the same bits; accumulate twice is exactly 2 x (every value doubles exactly)
    first = tr.array_covariance(rxe, txe, array_frequency=CU.F_A)["buffer"]
    again = tr.array_covariance(rxe, txe, array_frequency=CU.F_A)["buffer"]
    assert tr.torch.equal(_bits(first), _bits(again))
    out = first.clone()
    tr.array_covariance(rxe, txe, array_frequency=CU.F_A, out=out, accumulate=True)
    assert tr.torch.equal(out, 2 * first)
    v = abi.covariance_views(out.cpu().numpy(), tr.nrx, tr.ntx, 17, 5)
    assert not CU.hermitian_errors(v["rx"]) and not CU.hermitian_errors(v["tx"])
    with pytest.raises(ValueError, match="out"):
        tr.array_covariance(rxe, txe, array_frequency=CU.F_A, out=out[:-1])


@pytest.mark.parametrize("world", [2, 3])
def test_shards_accumulate_to_the_whole(world):
    """shards (chunk = 64) planted by global identity, summed with accumulate=True: the generic planting against the
    whole's terms within CU.TOL, the exact planting at tolerance 0"""
    c = K.small(K.C4_DOPPLER, 3000)
    tr = _tracer(c)
    tr.trace()
    T = PL.plant(tr, keyed=True)
    Tx = CU.plant_exact(tr, T)
    nrx, ntx, fa = tr.nrx, tr.ntx, tr.f_ghz * 1e9
    rxe, txe = _half_wavelength(tr, "4x1")
    tr.close()
    exe = CU.exact_elements(33)
    assert (CU.F32_MFMA_ERR * CU.total_power(T, nrx, ntx) <= CU.TOL / 8).all()
    g = x = None
    for r in range(world):
        ts = _tracer(c, rank=r, world=world, chunk=64)
        ts.trace()
        U = PL.plant(ts, keyed=True)
        g = ts.array_covariance(rxe, txe, out=g, accumulate=g is not None)["buffer"]
        CU.plant_exact(ts, U)
        x = ts.array_covariance(rx_elements=exe, array_frequency=CU.F_A, out=x, accumulate=x is not None)["buffer"]
        ts.torch.cuda.synchronize(ts.device)
        ts.close()
    got = abi.covariance_views(g.cpu().numpy(), nrx, ntx, 4, 1)
    for side, e in (("rx", rxe), ("tx", txe)):
        CU.check(got[side], CU.reference(T, nrx, ntx, e, fa, side), CU.TOL, "shards R_" + side, T, ntx)
    got = abi.covariance_views(x.cpu().numpy(), nrx, ntx, 33, 0)
    CU.check(got["rx"], CU.reference(Tx, nrx, ntx, exe, CU.F_A, "rx"), 0.0, "shards exact R_rx", Tx, ntx)


def test_link_without_terms_is_zero():
    tr = _small()
    counts = tr.counts()
    for b in range(tr.nb):   # every record of RX 0 blocked, and its LoS entries
        n = int(counts[b + 1])
        if n:
            keep = PL._mask_bits(tr, b, n)
            keep[0] = False
            PL._write_mask_bits(tr, b, n, keep)
    PL.los_view(tr).view(tr.torch.int32)[0, :, PL.LOS_STATUS] = 1
    tr.torch.cuda.synchronize(tr.device)
    T = CU.plant_exact(tr, PL.plant(tr))
    assert not (T["rx"] == 0).any() and (T["rx"] == 1).any()
    e = CU.exact_elements(65)
    got = _np(tr.array_covariance(e, e, array_frequency=CU.F_A))
    for side in ("rx", "tx"):
        assert not got[side][0].any(), side
        assert (np.abs(got[side][1]).reshape(tr.ntx, -1).max(axis=1) >= 1).all(), side
    CU.check(got["rx"], CU.reference(T, tr.nrx, tr.ntx, e, CU.F_A, "rx"), 0.0, "R_rx", T, tr.ntx)
    tr.close()


def test_scratch_too_small_is_refused():
    import torch
    tr = _tracer(K.small(K.C1, 2000))
    tr.trace()
    spec = abi.covariance_spec()
    d_el = torch.zeros(6, dtype=torch.float32, device=tr.device)
    a = abi.ArraySpec(1, 1, d_el.data_ptr(), d_el.data_ptr() + 12, CU.F_A)
    need = C.c_uint64(0)
    assert tr.L.hrt_array_covariance_scratch_bytes(tr.problem, C.byref(tr.shard), C.byref(spec), C.byref(a),
                                                   C.byref(need)) == 0
    scratch = torch.empty(int(need.value), dtype=torch.uint8, device=tr.device)
    out = torch.empty(abi.covariance_out_floats(1, 1, a, spec) // 2, dtype=torch.complex64, device=tr.device)
    rc = tr.L.hrt_array_covariance(tr.problem, C.byref(tr.shard), C.c_void_p(tr.ws.data_ptr()), C.byref(spec),
                                   C.byref(a), C.c_void_p(scratch.data_ptr()), C.c_uint64(int(need.value) - 1),
                                   C.c_void_p(out.data_ptr()), 0, None)
    assert rc == -1 and b"scratch" in tr.L.hrt_last_error()
    tr.close()


# ------------------------------------------------------------------ 6. poison
def test_poison_does_not_change_the_output():
    tr = _small()
    counts = tr.counts()
    _force_los_classes(tr)
    rxe, txe = _half_wavelength(tr, "2x2")

    def run():
        out = {p: _bits(tr.array_covariance(rxe, txe, los=p[0], scatter=p[1])["buffer"]) for p in PARTS}
        tr.torch.cuda.synchronize(tr.device)
        return out

    base = run()
    for p, b in base.items():
        assert bool(tr.torch.isfinite(b.view(tr.torch.float32)).all()), p
    for value in (float("nan"), 1e30):
        hit = PL.poison(tr, counts, value)
        for cls in ("blocked_records", "tail_slots", "tail_mask_bits", "los_blocked", "los_coincident"):
            assert hit[cls] > 0, (cls, hit)
        got = run()
        for p, b in base.items():
            assert bool(tr.torch.equal(got[p], b)), "covariance with %s changed after poison %r" % (p, value)
    tr.close()


# ------------------------------------------------------------------ 7. the drop-in entries
def test_drop_in_entries_match_the_tracer(product_lib):
    """hermespy_rt.compute_array_covariance and hrt_compute_array_covariance on host arrays trace the same rays and
    sum the same terms as the Tracer route; the batches of the drop-in may cut the records elsewhere, so the float32
    sums agree within the headroom of item 2 over the measured f32-MFMA error, 8 x 1.5e-7 x sum_p p"""
    import hermespy_rt_amd
    sys.path.insert(0, hermespy_rt_amd.LIB_DIR)
    import hermespy_rt
    c = K.small(K.C4_DOPPLER, 1100)
    tr = _tracer(c)
    tr.trace()
    rxe, txe = _half_wavelength(tr, "4x1")
    want = _np(tr.array_covariance(rxe, txe))
    rx_only = _np(tr.array_covariance(rx_elements=rxe))
    tr.close()
    d = abi.run_compute_array_covariance(product_lib, *K.args(c), abi.covariance_spec(), rxe, txe)
    nrx, ntx = len(c["rx_pos"]), len(c["tx_pos"])
    p = hermespy_rt.compute_array_covariance(
        c["scene_path"], np.array(c["rx_pos"], np.float32), np.array(c["tx_pos"], np.float32),
        np.array(c["rx_vel"], np.float32), np.array(c["tx_vel"], np.float32), c["f_ghz"], nrx, ntx, c["num_paths"],
        c["num_bounces"], rx_elements=rxe, tx_elements=txe)
    assert p["rx"].base is not None and p["rx"].shape == (nrx, ntx, 2, 4, 4) and p["tx"].shape == (nrx, ntx, 2, 1, 1)
    assert np.array_equal(p["buffer"], d["buffer"])
    P = want["tx"][..., 0, 0].real   # sum_p p of every link and polarisation
    assert (P > 0).any()
    for side in ("rx", "tx"):
        assert not CU.hermitian_errors(d[side]), side
        err = np.abs(d[side].astype(np.complex128) - want[side])
        assert (err <= 8 * CU.F32_MFMA_ERR * P[..., None, None]).all(), (side, err.max(), P.max())
    one = hermespy_rt.compute_array_covariance(
        c["scene_path"], np.array(c["rx_pos"], np.float32), np.array(c["tx_pos"], np.float32),
        np.array(c["rx_vel"], np.float32), np.array(c["tx_vel"], np.float32), c["f_ghz"], nrx, ntx, c["num_paths"],
        c["num_bounces"], rx_elements=rxe)
    assert one["tx"].size == 0 and one["buffer"].size == nrx * ntx * 2 * 16
    assert (np.abs(one["rx"].astype(np.complex128) - rx_only["rx"]) <= 8 * CU.F32_MFMA_ERR * P[..., None, None]).all()
    assert np.allclose(CV.correlation(one["rx"][P > 0])[..., 0, 0], 1.0)
