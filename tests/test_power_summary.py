"""hermespy_rt_amd.power.summarize against direct numpy statistics over synthetic path sets (no GPU)."""
import numpy as np
import pytest

from hermespy_rt_amd import abi, power

F = abi.POWER_FIELDS


def _moments(paths):
    """moments [2, F] of a list of (p_te, p_tm, tau, nu, u_rx, u_tx, is_los)"""
    m = np.zeros((2, F))
    for p_te, p_tm, tau, nu, urx, utx, los in paths:
        for pol, p in enumerate((p_te, p_tm)):
            m[pol, abi.POWER_COUNT] += 1
            m[pol, abi.POWER_P] += p
            m[pol, abi.POWER_P_TAU] += p * tau
            m[pol, abi.POWER_P_TAU2] += p * tau * tau
            m[pol, abi.POWER_P_NU] += p * nu
            m[pol, abi.POWER_P_NU2] += p * nu * nu
            m[pol, abi.POWER_P_URX_X:abi.POWER_P_URX_Z + 1] += p * np.asarray(urx)
            m[pol, abi.POWER_P_UTX_X:abi.POWER_P_UTX_Z + 1] += p * np.asarray(utx)
            m[pol, abi.POWER_P_LOS] += p if los else 0.0
    return m


def _unit(rng, n):
    u = rng.normal(size=(n, 3))
    return u / np.linalg.norm(u, axis=1, keepdims=True)


def _random_paths(rng, n, los=True):
    urx, utx = _unit(rng, n), _unit(rng, n)
    paths = [(rng.exponential(), rng.exponential(), rng.uniform(1e-8, 1e-6), rng.normal(0, 50.0), urx[i], utx[i],
              los and i == 0) for i in range(n)]
    return paths


def _direct(paths, pol):
    """the statistics straight from the paths: pol None combines both"""
    w = np.array([(p[0] + p[1]) if pol is None else p[pol] for p in paths])
    tau = np.array([p[2] for p in paths])
    nu = np.array([p[3] for p in paths])
    los = np.array([p[6] for p in paths])
    P = w.sum()
    d = {"num_paths": len(paths), "path_gain_db": 10 * np.log10(P)}
    d["mean_delay_s"] = np.average(tau, weights=w)
    d["rms_delay_spread_s"] = np.sqrt(np.average((tau - d["mean_delay_s"]) ** 2, weights=w))
    d["mean_doppler_hz"] = np.average(nu, weights=w)
    d["rms_doppler_spread_hz"] = np.sqrt(np.average((nu - d["mean_doppler_hz"]) ** 2, weights=w))
    for name, k in (("arrival", 4), ("departure", 5)):
        v = (w[:, None] * np.array([p[k] for p in paths])).sum(axis=0) / P
        r = np.linalg.norm(v)
        d["mean_%s_direction" % name] = v / r
        d["mean_%s_azimuth_rad" % name] = np.arctan2(v[1], v[0])
        d["mean_%s_zenith_rad" % name] = np.arccos(v[2] / r)
        d["%s_direction_spread" % name] = np.sqrt(1 - r * r)
    pl = w[los].sum()
    with np.errstate(divide="ignore"):
        d["k_factor_db"] = 10 * np.log10(pl / (P - pl))
    return d


@pytest.mark.parametrize("seed", range(5))
@pytest.mark.parametrize("pol", [None, 0, 1])
def test_summarize_matches_direct_statistics(seed, pol):
    rng = np.random.default_rng(seed)
    links = [_random_paths(rng, int(rng.integers(2, 40)), los=bool(seed % 2)) for _ in range(6)]
    m = np.stack([_moments(p) for p in links]).reshape(2, 3, 2, F)
    s = power.summarize(m, pol=pol)
    for i, paths in enumerate(links):
        want = _direct(paths, pol)
        for k, v in want.items():
            got = s[k].reshape((6,) + s[k].shape[2:])[i]
            if k == "k_factor_db" and not seed % 2:
                assert got == -np.inf
                continue
            assert np.allclose(got, v, rtol=1e-9, atol=1e-12 * (1e-6 if "delay" in k else 1.0)), (k, got, v)


def test_pol_combined_is_the_sum_of_the_pols():
    rng = np.random.default_rng(7)
    paths = _random_paths(rng, 17)
    m = _moments(paths)
    both = power.summarize(m)
    summed = np.zeros((2, F))
    summed[0] = m[0] + m[1]
    summed[0, abi.POWER_COUNT] = m[0, abi.POWER_COUNT]
    one = power.summarize(summed, pol=0)
    for k in both:
        assert np.allclose(both[k], one[k], rtol=1e-12), k
    assert both["num_paths"] == 17
    te, tm = power.summarize(m, pol=0), power.summarize(m, pol=1)
    assert np.isclose(10 ** (both["path_gain_db"] / 10), 10 ** (te["path_gain_db"] / 10) + 10 ** (tm["path_gain_db"] / 10))


def test_los_only_link():
    u = np.array([0.6, 0.0, 0.8])
    m = _moments([(0.25, 0.25, 3e-7, 12.0, -u, u, True)])
    s = power.summarize(m)
    assert s["k_factor_db"] == np.inf
    assert s["rms_delay_spread_s"] == 0 and s["rms_doppler_spread_hz"] == 0
    assert np.isclose(s["mean_delay_s"], 3e-7) and np.isclose(s["mean_doppler_hz"], 12.0)
    assert np.isclose(s["path_gain_db"], 10 * np.log10(0.5))
    assert np.allclose(s["mean_departure_direction"], u) and np.allclose(s["mean_arrival_direction"], -u)
    assert s["arrival_direction_spread"] < 1e-7 and s["departure_direction_spread"] < 1e-7
    assert np.isclose(s["mean_departure_zenith_rad"], np.arccos(0.8))
    assert np.isclose(s["mean_departure_azimuth_rad"], 0.0)


def test_all_zero_link():
    m = np.zeros((3, 2, F))
    m[1] = _moments(_random_paths(np.random.default_rng(1), 5))
    m[2, :, abi.POWER_COUNT] = 4   # terms of zero power
    s = power.summarize(m)
    assert s["path_gain_db"][0] == -np.inf and s["path_gain_db"][2] == -np.inf
    assert s["num_paths"][0] == 0 and s["num_paths"][2] == 4
    for k, v in s.items():
        if k in ("path_gain_db", "num_paths"):
            continue
        assert np.isnan(v[0]).all() and np.isnan(v[2]).all(), k
        assert np.isfinite(v[1]).all(), k


def test_accepts_torch_and_checks_the_shape():
    import torch
    m = _moments(_random_paths(np.random.default_rng(3), 9))
    a = power.summarize(torch.from_numpy(m))
    b = power.summarize(m)
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True)
    with pytest.raises(ValueError):
        power.summarize(np.zeros((2, F - 1)))
    with pytest.raises(ValueError):
        power.summarize(m, pol=2)
