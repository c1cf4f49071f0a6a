"""Host side of leaf folding (csrc/src/kernels/bitpar/leaf.hpp), no GPU: the decision function
and the n_core / leafw / parent-list builder against numpy, through the C API, and the
stand-alone self test under ASan + UBSan (csrc/tests/leaf_selftest.cpp, make -C csrc leaf-asan)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = os.path.join(ROOT, "build", "san")
CLASSES, PAD = 64, 256  # kLeafClasses, kLeafPad


def _degree_ordered(g):
    """The host graph renumbered by descending degree (stable), rows sorted."""
    deg = np.diff(g.rowptr)
    order = np.argsort(-deg, kind="stable")
    o2n = np.empty(g.n, np.int64)
    o2n[order] = np.arange(g.n)
    src = np.repeat(np.arange(g.n), deg)
    u, v = o2n[src], o2n[g.col]
    k = np.lexsort((v, u))
    rowptr = np.zeros(g.n + 1, np.int64)
    np.cumsum(np.bincount(u, minlength=g.n), out=rowptr[1:])
    return rowptr, v[k].astype(np.int32)


def _lists(native, n, rowptr, col):
    L = native.lib()
    info = np.zeros(8, np.int64)
    rp, cp = native.ptr(rowptr, C.c_int64), native.ptr(col, C.c_int32)
    native.check(L.msbfs_leaf_fold_lists(n, rp, cp, native.ptr(info, C.c_int64), None, 0, None,
                                         None, None))
    n_core, npos = int(info[0]), int(info[7])
    leafw = np.zeros(max(n_core, 1), np.int32)
    pidx = np.zeros(max(n_core, 1), np.int32)
    plist = np.zeros(max(npos, 1), np.int32)
    pw = np.zeros(max(npos, 1), np.int32)
    native.check(L.msbfs_leaf_fold_lists(n, rp, cp, native.ptr(info, C.c_int64),
                                         native.ptr(leafw, C.c_int32), npos,
                                         native.ptr(plist, C.c_int32), native.ptr(pw, C.c_int32),
                                         native.ptr(pidx, C.c_int32)))
    return info, leafw[:n_core], plist[:npos], pw[:npos], pidx[:n_core]


def _graphs(m):
    star = m.Graph.from_edges(700, np.zeros(699, np.int32), np.arange(1, 700, dtype=np.int32))
    return [("rmat12", m.Graph.rmat(12, 16, 1)), ("star", star), ("grid", m.Graph.grid(30, 40))]


@pytest.mark.parametrize("which", [0, 1, 2])
def test_lists_against_numpy(msbfs_pkg, which):
    m = msbfs_pkg
    from msbfs.ops import native
    name, g = _graphs(m)[which]
    rowptr, col = _degree_ordered(g)
    deg = np.diff(rowptr)
    info, leafw, plist, pw, pidx = _lists(native, g.n, rowptr, col)
    n_core, n_eff, parents, attached, max_w, nsmall, nheavy, npos = (int(x) for x in info)
    assert n_core == int((deg >= 2).sum()) and n_eff == int((deg >= 1).sum()), name
    # leafw = row entries >= n_core, per vertex below n_core
    src = np.repeat(np.arange(g.n), deg)
    want = np.bincount(src[col >= n_core], minlength=g.n)[:n_core]
    assert np.array_equal(leafw, want), name
    assert parents == int((want > 0).sum()) and attached == int(want.sum())
    assert max_w == (int(want.max()) if n_core else 0)
    assert nheavy == int((want > CLASSES).sum()) and nsmall % PAD == 0 and npos == nsmall + nheavy
    # the list: every parent once, at the position pidx says, with its weight; padding is -1
    listed = plist[plist >= 0]
    assert np.array_equal(np.sort(listed), np.flatnonzero(want > 0)), name
    assert np.array_equal(pw[plist >= 0], want[listed])
    assert np.array_equal(pidx[listed], np.flatnonzero(plist >= 0))
    assert np.all(pidx[want == 0] == -1)
    # classes: ascending weights, one weight per PAD positions, id order within a class
    small = pw[:nsmall].reshape(-1, PAD) if nsmall else np.zeros((0, PAD), np.int32)
    assert np.all(small == small[:, :1]) and np.all(np.diff(small[:, 0]) >= 0)
    assert np.all((small >= 1) & (small <= CLASSES))
    for c in np.unique(small[:, 0]) if nsmall else []:
        ids = plist[:nsmall][(pw[:nsmall] == c) & (plist[:nsmall] >= 0)]
        assert np.all(np.diff(ids) > 0)
    assert np.all(plist[nsmall:] >= 0) and np.all(pw[nsmall:] > CLASSES)
    if name == "star":
        assert (n_core, n_eff, parents, max_w, nheavy) == (1, 700, 1, 699, 1)
    if name == "grid":
        assert n_core == n_eff == g.n and parents == 0 and npos == 0
    if name == "rmat12":
        assert parents > 0 and 0.1 < (n_eff - n_core) / n_eff < 0.3


def test_lists_reject_unordered_degrees(msbfs_pkg):
    from msbfs.ops import native
    rowptr = np.array([0, 1, 3, 4], np.int64)  # degrees 1, 2, 1
    col = np.array([1, 0, 2, 1], np.int32)
    info = np.zeros(8, np.int64)
    with pytest.raises(native.MsbfsError):
        native.check(native.lib().msbfs_leaf_fold_lists(
            3, native.ptr(rowptr, C.c_int64), native.ptr(col, C.c_int32),
            native.ptr(info, C.c_int64), None, 0, None, None, None))


def test_decision(msbfs_pkg):
    from msbfs.ops import native
    on = native.lib().msbfs_leaf_fold_on
    # (leaf_key, relabelled, rows_sorted, count, nparts, limited, n_core, n_eff)
    assert on(-1, 1, 1, 0, 1, 0, 75, 100) == 1      # auto: a quarter are leaves
    assert on(-1, 1, 1, 0, 1, 0, 875, 1000) == 1    # exactly 1/8
    assert on(-1, 1, 1, 0, 1, 0, 876, 1000) == 0    # below it (grids, uniform graphs)
    assert on(1, 1, 1, 0, 1, 0, 999, 1000) == 1     # forced on: any leaf
    assert on(1, 1, 1, 0, 1, 0, 1000, 1000) == 0    # ... but there is none
    assert on(0, 1, 1, 0, 1, 0, 10, 1000) == 0      # off
    assert on(1, 0, 1, 0, 1, 0, 10, 1000) == 0      # the user's ids
    assert on(1, 1, 0, 0, 1, 0, 10, 1000) == 0      # unsorted rows
    assert on(1, 1, 1, 1, 1, 0, 10, 1000) == 0      # edge counting / distances / parents
    assert on(1, 1, 1, 0, 2, 0, 10, 1000) == 0      # a hybrid phase
    assert on(1, 1, 1, 0, 1, 1, 10, 1000) == 0      # a level limit
    assert on(1, 1, 1, 0, 1, 0, 10, 2 ** 31) == 0   # ids beyond int32


def test_leaf_selftest_asan():
    probe = subprocess.run(["make", "-C", os.path.join(ROOT, "csrc"), "san-probe-asan"],
                           capture_output=True, text=True, timeout=600)
    if probe.returncode != 0:
        pytest.skip(f"the host compiler has no ASan: {probe.stderr[-300:]}")
    b = subprocess.run(["make", "-C", os.path.join(ROOT, "csrc"), "leaf-asan"],
                       capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-2000:]
    env = dict(os.environ)
    env["ASAN_OPTIONS"] = "detect_leaks=1:abort_on_error=1"
    r = subprocess.run([os.path.join(SAN, "leaf_selftest_asan")], capture_output=True, text=True,
                       timeout=600, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "leaf selftest: ok" in r.stdout and "ERROR: AddressSanitizer" not in r.stderr
