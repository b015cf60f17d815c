"""Power statistics of links from the moments of Tracer.power_profiles / hermespy_rt.compute_power_profiles
(include/hermespy_rt.h hrt_compute_power_profiles).  Plain numpy; torch tensors are accepted.

    s = summarize(tr.power_profiles(0.0, 1e-8, 256)["moments"])
    s["rms_delay_spread_s"]      # [nrx, ntx]
"""
import numpy as np

from . import abi


def _np(a):
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    return np.asarray(a, np.float64)


def summarize(moments, pol=None):
    """Per-link statistics of moments [..., 2, POWER_FIELDS] (pol None: both polarisations combined, the P-weighted
    fields added and COUNT taken once; pol 0 = TE or 1 = TM: that one alone).  Returns a dict of float64 arrays over
    the leading axes (a trailing axis of 3 for the direction vectors):

        num_paths                      terms summed (COUNT)
        path_gain_db                   10 log10 P
        mean_delay_s, rms_delay_spread_s          tau weighted by p: mean, sqrt(E[tau^2] - mean^2)
        mean_doppler_hz, rms_doppler_spread_hz    the same for nu
        mean_arrival_direction, mean_departure_direction   unit vector of sum p u / P
        mean_arrival_azimuth_rad, mean_arrival_zenith_rad, mean_departure_azimuth_rad, mean_departure_zenith_rad
        arrival_direction_spread, departure_direction_spread   Fleury: sqrt(1 - |sum p u / P|^2)
        k_factor_db                    10 log10 (P_LOS / (P - P_LOS))

    Variances are clamped at 0.  P = 0 gives path_gain_db = -inf and NaN for every other statistic (num_paths
    stays); with no scatter power K = +inf."""
    m = _np(moments)
    if m.ndim < 2 or m.shape[-2:] != (2, abi.POWER_FIELDS):
        raise ValueError("moments must have shape (..., 2, %d), got %s" % (abi.POWER_FIELDS, m.shape))
    if pol is None:
        f = m.sum(axis=-2)
        f[..., abi.POWER_COUNT] = m[..., 0, abi.POWER_COUNT]
    elif pol in (0, 1):
        f = m[..., pol, :].copy()
    else:
        raise ValueError("pol must be None, 0 or 1")
    P = f[..., abi.POWER_P]
    live = P > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = np.where(live, 1.0 / np.where(live, P, 1.0), np.nan)

        def mean_var(k1, k2):
            mu = f[..., k1] * inv
            return mu, np.sqrt(np.maximum(f[..., k2] * inv - mu * mu, 0.0))

        out = {"num_paths": f[..., abi.POWER_COUNT],
               "path_gain_db": np.where(live, 10.0 * np.log10(np.where(live, P, 1.0)), -np.inf)}
        out["mean_delay_s"], out["rms_delay_spread_s"] = mean_var(abi.POWER_P_TAU, abi.POWER_P_TAU2)
        out["mean_doppler_hz"], out["rms_doppler_spread_hz"] = mean_var(abi.POWER_P_NU, abi.POWER_P_NU2)
        for name, k in (("arrival", abi.POWER_P_URX_X), ("departure", abi.POWER_P_UTX_X)):
            v = f[..., k:k + 3] * inv[..., None]
            r = np.sqrt((v * v).sum(axis=-1))
            u = v / r[..., None]
            out["mean_%s_direction" % name] = u
            out["mean_%s_azimuth_rad" % name] = np.arctan2(u[..., 1], u[..., 0])
            out["mean_%s_zenith_rad" % name] = np.arccos(np.clip(u[..., 2], -1.0, 1.0))
            out["%s_direction_spread" % name] = np.sqrt(np.maximum(1.0 - r * r, 0.0))
        los = f[..., abi.POWER_P_LOS]
        nlos = np.maximum(P - los, 0.0)
        k = np.where(nlos > 0, los / np.where(nlos > 0, nlos, 1.0), np.inf)
        out["k_factor_db"] = np.where(live, 10.0 * np.log10(k), np.nan)
    return out
