"""Antenna radiation patterns and orientations (include/hermespy_rt.h hrt_pattern; csrc/hrt_patterns.hip).

A pattern is a real field factor F >= 0 (sqrt of the gain) of the look direction in the antenna's local frame:
boresight +x, zenith theta from +z, azimuth phi = atan2(y, x).  An orientation is the 3 x 3 world -> local rotation R of
an endpoint.  Every unblocked scatter record and every clear LoS entry of a traced workspace is weighted by

    w = F_rx(R_rx[rx] u_rx) F_tx(R_tx[tx] u_tx)

with u_rx, u_tx the outward look directions of the path at its two ends (Tracer.set_patterns, the `patterns=` keyword
of the hermespy_rt path-sum functions).  A pattern is a plain dict(kind, gain_db, table):

    isotropic()        F = g                                         g = 10^(gain_db / 20)
    dipole()           half-wave dipole along local z, 2.15 dBi:     F = g sqrt(1.64) cos(pi/2 cos theta) / sin theta
    tr38901()          TR 38.901 table 7.3-1, 8 dBi, 65 deg beamwidths, 30 dB floor
    table(values)      [num_zenith, num_azimuth] amplitudes at theta_i = pi i / (num_zenith - 1) and
                       phi_k = -pi + 2 pi k / num_azimuth (periodic), bilinear

weight() is the float64 reference the device kernel is tested against."""
import numpy as np

ISOTROPIC, DIPOLE, TR38901, TABLE = 0, 1, 2, 3
MAX_ZENITH, MAX_AZIMUTH, MAX_GAIN_DB = 181, 360, 200.0
DIPOLE_SIN_MIN = 2.0 ** -12        # below it the dipole is its limit sqrt(1.64) (pi / 4) sin theta
ORTHONORMAL_TOL = 1e-5


def isotropic(gain_db=0.0):
    return dict(kind=ISOTROPIC, gain_db=float(gain_db), table=None)


def dipole(gain_db=0.0):
    return dict(kind=DIPOLE, gain_db=float(gain_db), table=None)


def tr38901(gain_db=0.0):
    return dict(kind=TR38901, gain_db=float(gain_db), table=None)


def table(values, gain_db=0.0):
    """values [num_zenith, num_azimuth] (2 .. 181 x 1 .. 360), finite and >= 0"""
    return check(dict(kind=TABLE, gain_db=float(gain_db), table=values))


def check(pattern):
    """the pattern as dict(kind, gain_db, table) with a contiguous float32 table; ValueError names what is wrong"""
    if pattern is None:
        return isotropic()
    try:
        kind, gain_db, values = int(pattern["kind"]), float(pattern["gain_db"]), pattern.get("table")
    except (TypeError, KeyError, ValueError):
        raise ValueError("a pattern is a dict(kind, gain_db, table): patterns.isotropic(), dipole(), tr38901(), table()")
    if not 0 <= kind <= TABLE:
        raise ValueError("pattern kind = %d (0 .. 3)" % kind)
    if not np.isfinite(gain_db) or abs(gain_db) > MAX_GAIN_DB:
        raise ValueError("gain_db must be finite and within +-200 dB")
    if kind != TABLE:
        return dict(kind=kind, gain_db=gain_db, table=None)
    if values is None:
        raise ValueError("a table pattern needs its table")
    v = np.ascontiguousarray(np.asarray(values.cpu().numpy() if hasattr(values, "cpu") else values, np.float32))
    if v.ndim != 2 or not 2 <= v.shape[0] <= MAX_ZENITH or not 1 <= v.shape[1] <= MAX_AZIMUTH:
        raise ValueError("a pattern table has shape (num_zenith 2 .. 181, num_azimuth 1 .. 360), got %s" % (v.shape,))
    if not np.isfinite(v).all() or (v < 0).any():
        raise ValueError("table values must be finite and >= 0")
    return dict(kind=kind, gain_db=gain_db, table=v)


def gain(pattern):
    """g = 10^(gain_db / 20) as the float the kernel multiplies by"""
    return np.float32(10.0 ** (float(pattern["gain_db"]) / 20.0))


# ------------------------------------------------------------------ orientations
def rotation(yaw=0.0, pitch=0.0, roll=0.0):
    """World -> local rotation (3 x 3 float32) of an antenna turned from the world axes by yaw about z, then pitch
    about the new y, then roll about the new x (radians): the local axes in world coordinates are the columns of
    Rz(yaw) Ry(pitch) Rx(roll), and this is its transpose.  The boresight is (cos yaw cos pitch, sin yaw cos pitch,
    -sin pitch): a positive pitch tilts it down."""
    cy, sy, cp, sp, cr, sr = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
    rz = np.array([[cy, -sy, 0.0], [sy, cy, 0.0], [0.0, 0.0, 1.0]])
    ry = np.array([[cp, 0.0, sp], [0.0, 1.0, 0.0], [-sp, 0.0, cp]])
    rx = np.array([[1.0, 0.0, 0.0], [0.0, cr, -sr], [0.0, sr, cr]])
    return np.ascontiguousarray((rz @ ry @ rx).T.astype(np.float32))


def look_at(direction, up=(0.0, 0.0, 1.0)):
    """World -> local rotation (3 x 3 float32) of an antenna whose boresight (local +x) points along `direction`, its
    local z as close to `up` as that allows (direction parallel to up: local y = world y)."""
    x = np.asarray(direction, np.float64).reshape(3)
    n = np.linalg.norm(x)
    if not np.isfinite(n) or n == 0.0:
        raise ValueError("look_at needs a finite direction that is not zero")
    x = x / n
    y = np.cross(np.asarray(up, np.float64).reshape(3), x)
    if np.linalg.norm(y) < 1e-9:
        y = np.cross(x, np.cross(np.array([0.0, 1.0, 0.0]), x))
        y = y if np.linalg.norm(y) > 1e-9 else np.array([0.0, 1.0, 0.0])
    y = y / np.linalg.norm(y)
    z = np.cross(x, y)
    return np.ascontiguousarray(np.stack([x, y, z]).astype(np.float32))


def orientations(R, n, name):
    """the orientations of n endpoints as a contiguous float32 [n, 3, 3] (one 3 x 3 serves them all); None stays None.
    ValueError unless every matrix is orthonormal within 1e-5."""
    if R is None:
        return None
    a = np.asarray(R.cpu().numpy() if hasattr(R, "cpu") else R, np.float32)
    if a.shape == (3, 3):
        a = np.broadcast_to(a, (n, 3, 3))
    if a.shape != (n, 3, 3):
        raise ValueError("%s must have shape (3, 3) or (%d, 3, 3), got %s" % (name, n, a.shape))
    a = np.ascontiguousarray(a)
    if not np.isfinite(a).all():
        raise ValueError("%s must be finite" % name)
    d = a.astype(np.float64)
    err = np.abs(d @ d.transpose(0, 2, 1) - np.eye(3)).max(initial=0.0)
    if err > ORTHONORMAL_TOL:
        raise ValueError("%s is not orthonormal within 1e-5 (R R^T - I up to %.3g)" % (name, err))
    return a


# ------------------------------------------------------------------ the float64 reference
def local(R, u):
    """R u in float64 (R None: u), every row summed left to right as the kernel does"""
    u = np.asarray(u, np.float64)
    if R is None:
        return u[..., 0], u[..., 1], u[..., 2]
    R = np.asarray(R, np.float64)
    return tuple((R[..., k, 0] * u[..., 0] + R[..., k, 1] * u[..., 1]) + R[..., k, 2] * u[..., 2] for k in range(3))


def angles(R, u):
    """zenith from local +z and azimuth atan2(y, x) of R u (float64)"""
    x, y, z = local(R, u)
    return np.arctan2(np.hypot(x, y), z), np.arctan2(y, x)


def table_value(values, theta, phi):
    """bilinear interpolation of values [num_zenith, num_azimuth] (float64), periodic in azimuth"""
    v = np.asarray(values, np.float64)
    nz, na = v.shape
    tz = np.asarray(theta, np.float64) * ((nz - 1) / np.pi)
    i0 = np.clip(np.floor(tz), 0, nz - 2).astype(np.int64)
    sz = np.minimum(tz - i0, 1.0)
    ta = (np.asarray(phi, np.float64) + np.pi) * (na / (2.0 * np.pi))
    k = np.floor(ta)
    sa = ta - k
    k0 = k.astype(np.int64) % na
    k1 = (k0 + 1) % na
    a = v[i0, k0] + sa * (v[i0, k1] - v[i0, k0])
    b = v[i0 + 1, k0] + sa * (v[i0 + 1, k1] - v[i0 + 1, k0])
    return a + sz * (b - a)


def weight(pattern, R, u):
    """F(R u) of one side in float64: pattern a dict of this module, R a 3 x 3 world -> local rotation (or [..., 3, 3],
    or None for the identity), u [..., 3] outward look directions in world coordinates (any length but zero).  The
    weight of a path is weight(rx, R_rx, u_rx) * weight(tx, R_tx, u_tx)."""
    p = check(pattern)
    g = 10.0 ** (p["gain_db"] / 20.0)
    theta, phi = angles(R, u)
    if p["kind"] == ISOTROPIC:
        return np.full(np.shape(theta), g)
    if p["kind"] == DIPOLE:
        s, c = np.sin(theta), np.cos(theta)
        with np.errstate(divide="ignore", invalid="ignore"):
            f = np.cos(0.5 * np.pi * c) / s
        return g * np.sqrt(1.64) * np.where(s < DIPOLE_SIN_MIN, 0.25 * np.pi * s, f)
    if p["kind"] == TR38901:
        av = -np.minimum(12.0 * ((np.degrees(theta) - 90.0) / 65.0) ** 2, 30.0)
        ah = -np.minimum(12.0 * (np.degrees(phi) / 65.0) ** 2, 30.0)
        a = -np.minimum(-(av + ah), 30.0)
        return g * 10.0 ** ((8.0 + a) / 20.0)
    return g * table_value(p["table"], theta, phi)
