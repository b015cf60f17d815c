"""What tests/test_covariance_design.py (no device) and tests/test_gpu_covariance.py share: the exact planting of the
spatial covariance matrices (Tracer.array_covariance), the float64 reference from planted terms, the wrong results a
kernel could give (MUTANTS) and the check.

The exact planting, on top of PL.plant (|a|^2 in {1/4, 1, 4}):

    f_a = 8 c Hz                          f_a / c = 8.0 exactly
    elements on (1/32 m) {0..7}^3         exact in float32; r . u for u on an axis is +-k / 32
    u_rx in {+-e_x, +-e_y, +-e_z}         by PL.mix of the record's global identity (as power_edges_util plants its
                                          direction classes); the direction of a clear LoS entry likewise

so every steering phase is a whole number of quarter revolutions, every s_i(u) is one of 1, j, -1, -j, and every entry
of R is a sum of integer multiples of 1/4 below 2^22: exact in float32 in any order.  u_tx of a scatter record is the
launch direction of its ray and cannot be planted, so R_tx is exact for the LoS part only.  Only plant_exact() needs a
device."""
import numpy as np

from hermespy_rt_amd import covariance as CV

from . import planted as PL

F_A = 8 * 299792458.0          # Hz: f_a / c = 8 revolutions per metre
STEP = 1.0 / 32.0              # the element lattice (m)
TILE = (16, 32)                # the MFMA tile of csrc/hrt_covariance.h: row elements x column elements
SIZES = (1, 15, 16, 17, 31, 32, 33, 64, 65, 256)
AXES = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float64)
TOL = 1.0 / 32.0               # generic planting: an eighth of the smallest planted p (1/4)
F32_MFMA_ERR = 1.5e-7          # of sum |a b|: the error of an f32-MFMA chain of up to 1 024 terms measured on gfx950


def exact_elements(n, salt=0):
    """float32 [n, 3]: n distinct points of the lattice (1/32 m) {0..7}^3, in an order set by PL.mix"""
    assert 1 <= n <= 512
    k = np.argsort(PL.mix(np.arange(512), 0xE1 + salt), kind="stable")[:n]
    e = np.stack([k & 7, (k >> 3) & 7, k >> 6], axis=1) * STEP
    return e.astype(np.float32)


def mirror_symmetric(e):
    """the axes in which the point set e (lattice {0..7}^3 / 32) is its own mirror image"""
    k = np.rint(np.asarray(e, np.float64) / STEP).astype(np.int64)
    have = {tuple(p) for p in k}
    out = []
    for ax in range(3):
        m = k.copy()
        m[:, ax] = 7 - m[:, ax]
        if {tuple(p) for p in m} == have:
            out.append(ax)
    return out


def axis_of(T, salt=0):
    """the axis class (index into AXES) of every term, from the hash of its global identity"""
    return ((PL.mix(T["rx"], T["tx"], T["path"], T["bounce"], 0xC0 + salt) >> np.uint64(17)) % np.uint64(6)).astype(
        np.int64)


def exact_values(T, fixed=None, salt=0):
    """T with u_rx (LoS terms: u_tx, and u_rx = -u_tx) on the axes; `fixed` marks terms left as they are (coincident
    LoS entries, whose directions are +-e_x by definition)"""
    u = AXES[axis_of(T, salt)]
    keep = np.zeros(u.shape[0], bool) if fixed is None else np.asarray(fixed, bool)
    los = T["los"] & ~keep
    U = {key: v.copy() for key, v in T.items()}
    U["urx"] = np.where(keep[:, None], T["urx"], np.where(los[:, None], -u, u))
    U["utx"] = np.where(los[:, None], u, T["utx"])
    return U


def plant_exact(tr, T, salt=0):
    """write exact_values into tr's workspace (after PL.plant(tr) returned T); returns the updated terms"""
    torch = tr.torch
    st = PL.los_status(tr)
    rx, tx = np.maximum(T["rx"], 0), np.maximum(T["tx"], 0)
    fixed = T["los"] & (st[rx, tx] != 2)
    U = exact_values(T, fixed, salt)
    sc = ~T["los"]
    for b in np.unique(T["bounce"][sc]):
        s = np.nonzero(sc & (T["bounce"] == b))[0]
        n = int(T["index"][s].max()) + 1
        blk = tr.rec_block(int(b))
        recs = blk[:, :, :n].cpu().numpy().view(np.float32).copy()
        r, i = T["rx"][s], T["index"][s]
        for q in range(3):
            recs[r, PL.REC_DIRX + q, i] = U["urx"][s, q]
        blk[:, :, :n] = torch.from_numpy(recs.view(np.int32)).to(tr.device)
    L = PL.los_view(tr)
    Lh = L.cpu().numpy().copy()
    for j in np.nonzero(T["los"] & ~fixed)[0]:
        Lh[T["rx"][j], T["tx"][j], PL.LOS_DIRX:PL.LOS_DIRZ + 1] = U["utx"][j]
    L.copy_(torch.from_numpy(Lh).to(tr.device))
    torch.cuda.synchronize(tr.device)
    return U


def powers(T):
    """[2, P]: p = |a^pol|^2 of every term"""
    return np.stack([np.abs(T["a_te"]) ** 2, np.abs(T["a_tm"]) ** 2])


def reference(T, nrx, ntx, elements, fa, side):
    """complex128 [nrx, ntx, 2, N, N]: R_rx (side "rx": u_rx) or R_tx (side "tx": u_tx) of the terms T, by
    hermespy_rt_amd.covariance.from_terms link by link"""
    e = np.asarray(elements, np.float32).astype(np.float64).reshape(-1, 3)
    R = np.zeros((nrx, ntx, 2, e.shape[0], e.shape[0]), np.complex128)
    link = PL.link_of(T, ntx)
    p, u = powers(T), T["urx" if side == "rx" else "utx"]
    for lk in np.unique(link):
        s = link == lk
        R[lk // ntx, lk % ntx] = CV.from_terms(p[:, s], u[s], e, fa)
    return R


def total_power(T, nrx, ntx):
    """[nrx, ntx, 2]: sum_p p of every link"""
    p = powers(T)
    nl = nrx * ntx
    return np.stack([np.bincount(PL.link_of(T, ntx), weights=p[q], minlength=nl) for q in range(2)],
                    axis=1).reshape(nrx, ntx, 2)


# ------------------------------------------------------------------ the wrong results (negative controls)
def _swap_dirs(T):
    U = {key: v.copy() for key, v in T.items()}
    U["urx"], U["utx"] = T["utx"].copy(), T["urx"].copy()
    return U


def _swap_pols(T):
    U = {key: v.copy() for key, v in T.items()}
    U["a_te"], U["a_tm"] = T["a_tm"].copy(), T["a_te"].copy()
    return U


def _los_same_side(T):
    U = {key: v.copy() for key, v in T.items()}
    U["urx"][T["los"]] = T["utx"][T["los"]]
    return U


def _drop_last_element(R):
    R = R.copy()
    R[..., -1, :] = 0
    R[..., :, -1] = 0
    return R


def _one_tile_off(R):
    """every 16 x 32 tile written one tile to the right (what falls off the matrix is lost, the first tile column
    stays empty)"""
    out = np.zeros_like(R)
    out[..., :, TILE[1]:] = R[..., :, :-TILE[1]]
    return out


def _diagonal_residue(R):
    """the diagonal as the MFMA's fmaf chain leaves it: an imaginary part of one rounding of the real part"""
    R = R.copy()
    i = np.arange(R.shape[-1])
    R[..., i, i] += 1j * 2.0 ** -24 * R[..., i, i].real
    return R


# name -> (on: "terms" or "output", the change)
MUTANTS = {
    "transposed": ("output", lambda R: R.swapaxes(-1, -2).copy()),
    "conjugated": ("output", np.conj),
    "urx_utx_swapped": ("terms", _swap_dirs),
    "te_tm_swapped": ("terms", _swap_pols),
    "last_element_dropped": ("output", _drop_last_element),
    "one_tile_off": ("output", _one_tile_off),
    "diagonal_not_real": ("output", _diagonal_residue),
    "los_same_side": ("terms", _los_same_side),
}
# the mutants that cannot move anything in a 1 x 1 matrix (it is sum_p p whatever the directions are)
NEED_TWO_ELEMENTS = ("transposed", "conjugated", "urx_utx_swapped", "los_same_side")


def mutant(name, T, nrx, ntx, elements, fa, side):
    """the reference with the mutant `name` applied"""
    on, f = MUTANTS[name]
    if on == "terms":
        return reference(f(T), nrx, ntx, elements, fa, side)
    return f(reference(T, nrx, ntx, elements, fa, side))


# ------------------------------------------------------------------ the check
def hermitian_errors(R):
    """what is not Hermitian to the bit in R [..., N, N] (empty: nothing): every R[k, i] must equal conj(R[i, k]) as
    IEEE values (the sign of a zero aside) and every diagonal element must have imaginary part 0"""
    R = np.asarray(R)
    errs = []
    if not np.array_equal(R, np.conj(R).swapaxes(-1, -2)):
        errs.append("R != R^H")
    if np.any(np.diagonal(R, axis1=-2, axis2=-1).imag != 0):
        errs.append("diagonal not real")
    return errs


def check(got, ref, tol, what, T=None, ntx=None):
    """got [nrx, ntx, 2, N, N] (complex64) against ref within tol everywhere, the diagonal's imaginary part at
    tolerance 0 (it is 0 by definition), and got Hermitian to the bit; returns the largest |error|"""
    got = np.asarray(got)
    assert not hermitian_errors(got), (what, hermitian_errors(got))
    i = np.arange(ref.shape[-1])
    assert np.array_equal(got[..., i, i].imag, ref[..., i, i].imag), (what, "imaginary part of the diagonal")
    return PL.check_close(got, ref, tol, what, T, ntx)
