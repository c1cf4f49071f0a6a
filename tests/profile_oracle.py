"""The oracle of the level-profile tests (test_profile_cpu.py, test_profile_gpu.py), independent
of the profile code: np.bincount over the rows of the distance matrix cpu_bfs(distances=True)
returns, with the tail folded into the last bin here."""
import numpy as np


def fold(hist_full, nbins):
    """A histogram with a column per level -> `nbins` columns, the last one the tail."""
    H = np.asarray(hist_full, np.int64)
    out = np.zeros((H.shape[0], nbins), np.int64)
    k = min(nbins - 1, H.shape[1])
    out[:, :k] = H[:, :k]
    out[:, nbins - 1] += H[:, k:].sum(axis=1) if nbins - 1 < H.shape[1] else 0
    return out


def from_distances(dist):
    """(F, reach, ecc, hist with max(ecc) + 2 columns: the last one is zero) of a distance matrix"""
    D = np.asarray(dist)
    K = D.shape[0]
    top = int(D.max()) if D.size else -1
    H = np.zeros((K, max(top, -1) + 2), np.int64)
    F = np.zeros(K, np.int64)
    reach = np.zeros(K, np.int64)
    ecc = np.full(K, -1, np.int32)
    for k in range(K):
        d = D[k][D[k] >= 0].astype(np.int64)
        F[k] = d.sum()
        reach[k] = len(d)
        if len(d):
            ecc[k] = d.max()
            b = np.bincount(d)
            H[k, :len(b)] = b
    return F, reach, ecc, H


def oracle(m, g, qs):
    return from_distances(m.cpu_bfs(g, qs, distances=True).dist)


def check(res, ora, nbins, what=""):
    """A profile result against the oracle tuple, exact, plus the contract's own identities."""
    F, reach, ecc, H = ora
    assert np.array_equal(res.F, F), (what, "F", np.flatnonzero(res.F != F)[:8])
    assert res.reach.dtype == np.int64 and res.ecc.dtype == np.int32 and res.hist.dtype == np.int64
    assert np.array_equal(res.reach, reach), (what, "reach", np.flatnonzero(res.reach != reach)[:8],
                                              res.reach[res.reach != reach][:8],
                                              reach[res.reach != reach][:8])
    assert np.array_equal(res.ecc, ecc), (what, "ecc", np.flatnonzero(res.ecc != ecc)[:8],
                                          res.ecc[res.ecc != ecc][:8], ecc[res.ecc != ecc][:8])
    assert res.hist.shape == (len(F), nbins), (what, res.hist.shape)
    want = fold(H, nbins)
    bad = np.flatnonzero((res.hist != want).any(axis=1))
    assert len(bad) == 0, (what, "hist", bad[:8], res.hist[bad[:2]], want[bad[:2]])
    assert np.array_equal(res.hist.sum(axis=1), res.reach), what
    for k in np.flatnonzero(res.ecc < nbins - 1):
        e = int(res.ecc[k])
        assert (res.hist[k] * np.arange(nbins)).sum() == res.F[k], (what, k)
        assert e < 0 or res.hist[k, e] > 0, (what, k)
        assert not res.hist[k, e + 1:].any(), (what, k)
