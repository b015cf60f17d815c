"""The host side of the dominant paths (hermespy_rt_amd.dominant) on synthetic term lists (planted.synthetic_terms:
two power levels per link, so the tie-break decides almost every comparison): the order is strict, the merge of the
parts' lists is the list of the whole in every order, and the captured fraction closes."""
import itertools

import numpy as np
import pytest

from hermespy_rt_amd import abi, dominant

from . import planted as PL

NRX, NTX, PER_LINK = 2, 3, 300


def _terms(seed=0):
    T = PL.synthetic_terms(NRX, NTX, PER_LINK, seed=seed)
    # (bounce, path) is unique within a link in a trace; synthetic_terms draws paths at random: make them so
    T["path"] = np.where(T["los"], -1, np.arange(T["path"].size) * 7919 % (1 << 20))
    return T


def _same(a, b):
    assert np.array_equal(np.asarray(a["buffer"]), np.asarray(b["buffer"]))


@pytest.mark.parametrize("K", [1, 7, 64, 1024])
def test_reference_is_a_strict_order(K):
    T = _terms()
    R = dominant.reference(T, NRX, NTX, K)
    p = np.abs(T["a_te"]) ** 2 + np.abs(T["a_tm"]) ** 2
    assert np.unique(p).size <= 4   # few power levels: ties everywhere
    for rx in range(NRX):
        for tx in range(NTX):
            n = int(((T["rx"] == rx) & (T["tx"] == tx)).sum())
            kept = int(R["kept"][rx, tx])
            assert int(R["eligible"][rx, tx]) == n and kept == min(K, n)
            pw, b = R["power"][rx, tx, :kept], R["bounce"][rx, tx, :kept].astype(np.int64)
            path = R["path"][rx, tx, :kept]
            for i in range(kept - 1):   # every neighbour pair strictly ordered
                assert (pw[i] > pw[i + 1] or (pw[i] == pw[i + 1] and (b[i] < b[i + 1] or (
                    b[i] == b[i + 1] and path[i] < path[i + 1]))))
            # the kept set: nothing left out precedes the last kept term
            s = (T["rx"] == rx) & (T["tx"] == tx)
            key = sorted(zip(-p[s], T["bounce"][s], T["path"][s].astype(np.int64).view(np.uint64)))[:kept]
            assert [(-x, y, z) for x, y, z in key] == list(zip(pw, b, path))
            assert not R["power"][rx, tx, kept:].any() and not R["u_tx"][rx, tx, kept:].any()
    los = R["bounce"] == -1
    assert (R["path"][los] == dominant.LOS_PATH).all()
    assert np.array_equal(R["a_te"][los], R["a_tm"][los])


@pytest.mark.parametrize("K", [1, 64, 1024])
@pytest.mark.parametrize("nparts", [1, 2, 3, 4, 5])
def test_merge_of_parts_is_the_whole(K, nparts):
    T = _terms(seed=nparts)
    whole = dominant.reference(T, NRX, NTX, K)
    rng = np.random.default_rng(100 * K + nparts)
    part = rng.integers(0, nparts, T["rx"].size)
    lists = [dominant.reference(PL.select(T, part == q), NRX, NTX, K) for q in range(nparts)]
    for order in itertools.permutations(range(nparts)):
        acc = lists[order[0]]
        for q in order[1:]:
            acc = dominant.merge(acc, lists[q])
        _same(acc, whole)
    _same(dominant.merge(whole, dominant.empty(NRX, NTX, K)), whole)


def test_captured_fraction():
    T = _terms()
    p = np.stack([np.abs(T["a_te"]) ** 2, np.abs(T["a_tm"]) ** 2], axis=1)
    link = T["rx"] * NTX + T["tx"]
    M = np.zeros((NRX, NTX, 2, abi.POWER_FIELDS))
    for pol in range(2):
        M[:, :, pol, abi.POWER_P] = np.bincount(link, weights=p[:, pol], minlength=NRX * NTX).reshape(NRX, NTX)
    full = dominant.captured_fraction(dominant.reference(T, NRX, NTX, 1024), M)
    assert (full == 1.0).all()   # K >= eligible: everything is kept
    few = dominant.captured_fraction(dominant.reference(T, NRX, NTX, 7), M)
    assert ((few > 0) & (few < 1)).all()
    one, seven = dominant.reference(T, NRX, NTX, 1), dominant.reference(T, NRX, NTX, 7)
    assert (dominant.captured_fraction(one, M) < few).all() and (seven["kept"] == 7).all()
    assert np.isnan(dominant.captured_fraction(dominant.empty(1, 1, 4), np.zeros((1, 1, 2, abi.POWER_FIELDS)))).all()
