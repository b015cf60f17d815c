"""The antenna patterns on the host (hermespy_rt_amd.patterns): the float64 weight() against independent evaluations, the
orientation helpers, the float32 floor of the kernel's evaluation sequence (tests/patterns_util.py), and the wrong
readings of the definition, each caught by the planted cases.  No device."""
import math

import numpy as np
import pytest

from hermespy_rt_amd import patterns as P

from . import patterns_util as U


def _dir(theta_deg, phi_deg):
    t, p = math.radians(theta_deg), math.radians(phi_deg)
    return np.array([math.sin(t) * math.cos(p), math.sin(t) * math.sin(p), math.cos(t)])


def _db(f):
    return 20.0 * math.log10(float(f))


# ------------------------------------------------------------------ weight() against independent evaluations
def test_tr38901_boresight_halfpower_and_floors():
    p = P.tr38901()
    assert _db(P.weight(p, None, _dir(90, 0))) == pytest.approx(8.0, abs=1e-12)
    assert _db(P.weight(P.tr38901(3.0), None, _dir(90, 0))) == pytest.approx(11.0, abs=1e-12)
    # A = -12 (32.5 / 65)^2 = -3 dB at half the 65 degree beamwidth, in either plane and on either side
    for d in (_dir(90, 32.5), _dir(90, -32.5), _dir(57.5, 0), _dir(122.5, 0)):
        assert _db(P.weight(p, None, d)) == pytest.approx(5.0, abs=1e-9)
    assert _db(P.weight(p, None, _dir(57.5, 32.5))) == pytest.approx(2.0, abs=1e-9)
    # the floors: the horizontal cut is limited to 30 dB (from 102.8 degrees on), and so is the sum of the two cuts
    # (60 degrees off in zenith and 90 in azimuth: 10.2 + 23.0 dB); the vertical cut alone ends at 23.0 dB on the poles
    for d in (_dir(90, 180), _dir(90, 120), _dir(10, 170), _dir(90, -103), _dir(150, 90), _dir(30, -90)):
        assert _db(P.weight(p, None, d)) == pytest.approx(-22.0, abs=1e-9)
    for d in (np.array([0.0, 0.0, 1.0]), np.array([0.0, 0.0, -3.0])):
        assert _db(P.weight(p, None, d)) == pytest.approx(8.0 - 12 * (90 / 65) ** 2, abs=1e-9)
    assert _db(P.weight(p, None, _dir(90, 100))) == pytest.approx(8.0 - 12 * (100 / 65) ** 2, abs=1e-9)
    # the length of u does not matter
    assert P.weight(p, None, 7.5 * _dir(70, 20)) == pytest.approx(float(P.weight(p, None, _dir(70, 20))), rel=1e-14)


def test_dipole_maximum_and_pole_limit():
    p = P.dipole()
    for phi in (0, 77, -140):
        assert _db(P.weight(p, None, _dir(90, phi))) == pytest.approx(10 * math.log10(1.64), abs=1e-12)   # 2.15 dBi
    assert abs(_db(P.weight(p, None, _dir(90, 0))) - 2.15) < 0.005
    assert float(P.weight(p, None, _dir(60, 5))) == pytest.approx(math.sqrt(1.64) * math.cos(math.pi / 4) / math.sin(math.pi / 3))
    assert float(P.weight(p, None, np.array([0.0, 0.0, 1.0]))) == 0.0
    assert float(P.weight(p, None, np.array([0.0, 0.0, -2.0]))) == pytest.approx(0.0, abs=1e-15)
    # either side of sin(theta) = 2^-12 the limit and the formula agree far below the float32 floor
    for s in (2.0 ** -12 * 0.999, 2.0 ** -12 * 1.001, 1e-6, 1e-3):
        for z in (1.0, -1.0):
            got = float(P.weight(p, None, np.array([s, 0.0, z * math.sqrt(1 - s * s)])))
            assert got == pytest.approx(math.sqrt(1.64) * math.pi / 4 * s, rel=1e-6)
    assert float(P.weight(P.dipole(6.0), None, _dir(90, 0))) == pytest.approx(math.sqrt(1.64) * 10 ** 0.3)


def test_table_nodes_midpoints_wrap_and_single_azimuth():
    v = U.random_table(5, 8, 4)
    p = P.table(v)
    for i in range(5):
        for k in range(8):
            th, ph = 180.0 * i / 4, -180.0 + 360.0 * k / 8
            if i in (0, 4):
                continue   # (at a pole every azimuth is the same direction: below)
            assert float(P.weight(p, None, _dir(th, ph))) == pytest.approx(float(v[i, k]), rel=1e-12)
    # midpoints: the mean of the two or four nodes around
    assert float(P.weight(p, None, _dir(45 + 22.5, -180 + 45 * 3))) == pytest.approx((v[1, 3] + v[2, 3]) / 2, rel=1e-12)
    assert float(P.weight(p, None, _dir(90, -180 + 45 * 2.5))) == pytest.approx((v[2, 2] + v[2, 3]) / 2, rel=1e-12)
    assert float(P.weight(p, None, _dir(112.5, 22.5))) == pytest.approx(v[2:4, 4:6].mean(), rel=1e-12)
    # azimuth wrap-around: between the last node (135 degrees) and the first (-180 = 180 degrees)
    assert float(P.weight(p, None, _dir(90, 157.5))) == pytest.approx((v[2, 7] + v[2, 0]) / 2, rel=1e-12)
    assert float(P.weight(p, None, _dir(90, 180 - 1e-9))) == pytest.approx(float(v[2, 0]), rel=1e-9)
    assert float(P.weight(p, None, _dir(90, -180 + 1e-9))) == pytest.approx(float(v[2, 0]), rel=1e-9)
    assert float(P.weight(p, None, _dir(90, 168.75))) == pytest.approx(0.25 * v[2, 7] + 0.75 * v[2, 0], rel=1e-12)
    # the poles: phi = atan2(0, 0) = 0 is node 4
    assert float(P.weight(p, None, np.array([0.0, 0.0, 1.0]))) == float(v[0, 4])
    assert float(P.weight(p, None, np.array([0.0, 0.0, -1.0]))) == pytest.approx(float(v[4, 4]), rel=1e-12)
    # num_azimuth = 1: a function of the zenith alone; num_zenith = 2: linear from pole to pole
    one = P.table(np.array([[0.25], [1.5]], np.float32), gain_db=20.0)
    for th in (0, 30, 90, 135.5, 180):
        for ph in (-180, -33, 0, 179.9):
            assert float(P.weight(one, None, _dir(th, ph))) == pytest.approx(10 * (0.25 + 1.25 * th / 180), rel=1e-12)
    # a constant table returns its constant exactly, in float64 and in the kernel's float32 sequence
    R, u = U.cases(2000)
    for c in (0.5, 2.0 ** -3, 0.0, 1.7):
        const = P.table(np.full((181, 360), c, np.float32))
        assert np.all(P.weight(const, R, u) == np.float32(c))
        assert np.all(U.weight32(const, R, u) == np.float32(c))


def test_table_and_pattern_arguments_are_checked():
    for bad in (np.zeros((1, 4)), np.zeros((182, 4)), np.zeros((4, 0)), np.zeros((4, 361)), np.zeros(4),
                np.full((3, 3), -1e-3), np.full((3, 3), np.nan), np.full((3, 3), np.inf)):
        with pytest.raises(ValueError):
            P.table(bad)
    for bad in (dict(kind=4, gain_db=0.0), dict(kind=0, gain_db=math.nan), dict(kind=0, gain_db=200.5),
                dict(kind=3, gain_db=0.0), dict(gain_db=0.0), "dipole"):
        with pytest.raises(ValueError):
            P.check(bad)
    assert P.check(None) == P.isotropic()
    assert P.table(np.ones((181, 360)))["table"].dtype == np.float32
    assert P.gain(P.isotropic(20.0)) == np.float32(10.0) and P.gain(P.isotropic(-200.0)) == np.float32(1e-10)


# ------------------------------------------------------------------ orientations
def _rz(a):
    return np.array([[math.cos(a), -math.sin(a), 0], [math.sin(a), math.cos(a), 0], [0, 0, 1]])


def _ry(a):
    return np.array([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]])


def _rx(a):
    return np.array([[1, 0, 0], [0, math.cos(a), -math.sin(a)], [0, math.sin(a), math.cos(a)]])


def test_rotation_is_orthonormal_and_composes():
    rng = np.random.default_rng(5)
    for yaw, pitch, roll in rng.uniform(-math.pi, math.pi, (50, 3)):
        R = P.rotation(yaw, pitch, roll)
        assert R.dtype == np.float32 and R.shape == (3, 3) and R.flags["C_CONTIGUOUS"]
        assert np.abs(R.astype(np.float64) @ R.T.astype(np.float64) - np.eye(3)).max() < 1e-6
        assert np.linalg.det(R.astype(np.float64)) == pytest.approx(1.0, abs=1e-6)
        assert np.allclose(R, (_rz(yaw) @ _ry(pitch) @ _rx(roll)).T, atol=1e-7)
        # the boresight in world coordinates is the first row
        assert np.allclose(R[0], [math.cos(yaw) * math.cos(pitch), math.sin(yaw) * math.cos(pitch), -math.sin(pitch)],
                           atol=1e-7)
    assert np.array_equal(P.rotation(), np.eye(3, dtype=np.float32))
    # composition: turning by yaw a then yaw b is yaw a + b; the world -> local matrices multiply in reverse
    a, b = 0.4, -1.3
    assert np.allclose(P.rotation(b).astype(np.float64) @ P.rotation(a).astype(np.float64), P.rotation(a + b), atol=1e-6)
    # a yawed antenna sees a path along its boresight at local +x
    assert np.allclose(P.rotation(0.9) @ np.array([math.cos(0.9), math.sin(0.9), 0], np.float32), [1, 0, 0], atol=1e-6)
    P.orientations(np.stack([P.rotation(*v) for v in rng.uniform(-3, 3, (4, 3))]), 4, "R")


def test_look_at_points_the_boresight():
    rng = np.random.default_rng(6)
    for d in list(rng.normal(size=(50, 3))) + [np.array([0, 0, 2.0]), np.array([0, 0, -1.0]), np.array([1e-12, 0, 1.0])]:
        R = P.look_at(d)
        assert R.dtype == np.float32 and np.abs(R.astype(np.float64) @ R.T.astype(np.float64) - np.eye(3)).max() < 1e-6
        assert np.linalg.det(R.astype(np.float64)) == pytest.approx(1.0, abs=1e-6)
        assert np.allclose(R @ (d / np.linalg.norm(d)).astype(np.float32), [1, 0, 0], atol=1e-6)
        if abs(d[2]) < 0.999 * np.linalg.norm(d):
            assert R[2, 2] > 0 and abs(R[1, 2]) < 1e-7   # local z leans to world up, local y is horizontal
        assert float(P.weight(P.tr38901(), R, d)) == pytest.approx(10 ** 0.4, rel=1e-5)
        assert float(P.weight(P.tr38901(), R, -d)) == pytest.approx(10 ** -1.1, rel=1e-5)
    assert np.allclose(P.look_at([1, 1, 0]), P.rotation(math.pi / 4), atol=1e-7)
    assert np.allclose(P.look_at([1, 0, -1]), P.rotation(0, math.pi / 4), atol=1e-7)
    for bad in ([0, 0, 0], [math.nan, 0, 1]):
        with pytest.raises(ValueError):
            P.look_at(bad)


def test_orientations_are_checked():
    R = P.rotation(0.1, 0.2, 0.3)
    assert P.orientations(None, 3, "R") is None
    assert P.orientations(R, 3, "R").shape == (3, 3, 3)
    for bad in (R[:2], np.stack([R, R]), 1.0001 * R, R + np.float32(2e-5), np.full((3, 3), np.nan)):
        with pytest.raises(ValueError):
            P.orientations(bad, 3, "R")
    skew = R.copy()
    skew[0, 1] += 5e-6
    P.orientations(skew, 3, "R")   # within 1e-5


# ------------------------------------------------------------------ the float32 floor
def test_float32_floor_is_what_the_util_records():
    m = U.measured_floor()
    worst = max(m.values())
    print("float32 floor by pattern:", {k: "%.3g" % v for k, v in m.items()})
    assert worst <= U.FLOOR <= 2 * worst, (worst, U.FLOOR)
    assert U.TOL == 4 * U.FLOOR
    assert m["isotropic"] < 1e-7   # only g's rounding to float


def test_cases_cover_the_special_directions():
    R, u = U.special_cases()
    assert u.dtype == np.float32 and len(U.exact_rotations()) == 24
    x, y, z = U.local32(R, u)
    d = np.stack([x, y, z], axis=1).reshape(24, -1, 3)
    assert all(np.array_equal(d[k], U.special_local()) for k in range(24))   # exact: on the poles, axes and seam
    assert np.array_equal(np.stack(P.local(R, u), axis=1).reshape(24, -1, 3)[5], U.special_local().astype(np.float64))
    th, ph = P.angles(R, u)
    assert (th == 0).any() and (th == math.pi).any() and (ph == math.pi).any() and (ph < -3.14159).any()


def test_emulation_follows_the_dipole_threshold_and_the_seam():
    s = np.float32(2.0 ** -12)
    u = np.array([[s, 0, 1], [np.nextafter(s, np.float32(0)), 0, 1], [s * 2, 0, -1]], np.float32)
    for p in (P.dipole(), P.dipole(4.0)):
        assert np.allclose(U.weight32(p, None, u), P.weight(p, None, u), rtol=1e-6, atol=0)
    v = U.random_table(3, 360, 9)
    seam = np.array([[-1, 2.0 ** -22, 0.1], [-1, -(2.0 ** -22), 0.1], [-1, 0, 0.1], [-1, -0.0, 0.1]], np.float32)
    got, ref = U.weight32(P.table(v), None, seam), P.weight(P.table(v), None, seam)
    assert np.allclose(got, ref, rtol=0, atol=2e-5 * 2)


# ------------------------------------------------------------------ wrong readings
def test_the_right_reading_agrees_with_weight():
    rx, tx, R_rx, R_tx, u_rx, u_tx = U.wrong_reading_cases()
    right = U.link_weight(rx, tx, R_rx, R_tx, u_rx, u_tx)
    ref = P.weight(rx, R_rx, u_rx) * P.weight(tx, R_tx, u_tx)
    assert np.allclose(right, ref, rtol=1e-12, atol=0)
    w32 = U.weight32(rx, R_rx, u_rx) * U.weight32(tx, R_tx, u_tx)
    assert w32.dtype == np.float32
    assert np.all(np.abs(w32 - ref) <= U.weight_tolerance(rx, tx, P.weight(rx, R_rx, u_rx), P.weight(tx, R_tx, u_tx)))


@pytest.mark.parametrize("wrong", U.WRONG)
def test_wrong_reading_is_caught(wrong):
    rx, tx, R_rx, R_tx, u_rx, u_tx = U.wrong_reading_cases()
    f_rx, f_tx = P.weight(rx, R_rx, u_rx), P.weight(tx, R_tx, u_tx)
    tol = U.weight_tolerance(rx, tx, f_rx, f_tx)
    got = U.link_weight(rx, tx, R_rx, R_tx, u_rx, u_tx, **{wrong: True})
    assert (np.abs(got - f_rx * f_tx) > 100 * tol).any(), wrong
