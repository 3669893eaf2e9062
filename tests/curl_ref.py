"""Inputs of the CURL limits tests (tests/test_ngu_curl_limits_{gpu,host}.py): fp32 queries, keys and bilinear form whose
float64 logits decide every row's arg-max by MARGIN -- as test_curl_gpu._case demands of its own cases -- plus the planted
rows and the exact ties.  The reference itself stays test_curl_gpu._infonce64 under float64 autograd."""
import functools

import numpy as np

F32, F64 = np.float32, np.float64
MARGIN = 1e-4
TILE = 32                                       # ARL_CURL_TILE: query rows per tile = keys per tile
PLANTED_ROW = 5                                 # the row whose maximum is the last key
# (r, p): key p is a bitwise copy of key r, and both logits are row r's maximum: a hit only where r < p.  Three hits
# (across key tiles, inside one, first tile to last) and one miss: an arg-max that takes the LAST maximum gives 1, not 3
TIES = ((3, 40), (36, 37), (1, 63), (50, 7))


def logits64(zq, zk, w):
    return zq.astype(F64) @ w.astype(F64) @ zk.astype(F64).T


def margins(s):
    """every row's largest logit minus its second largest"""
    rest = s.copy()
    rest[np.arange(s.shape[0]), s.argmax(axis=1)] = -np.inf
    return s.max(axis=1) - rest.max(axis=1)


def settle(rs, zq, zk, w, fixed=(), copies=()):
    """Redraws (from rs, in place) every query row outside `fixed` whose two largest float64 logits are within MARGIN.
    copies: (r, p) pairs, key p a bitwise copy of key r -- column p takes column r's values (equal keys give equal
    logits), stays out of the comparison, and row p may not have its maximum there.  -> the float64 logits"""
    s = logits64(zq, zk, w)
    rows = np.arange(zq.shape[0])                                   # the rows still to look at
    keep = np.ones(zq.shape[0], bool)
    keep[[p for _, p in copies]] = False
    for _ in range(100):
        for r, p in copies:
            s[rows, p] = s[rows, r]
        sub = s[rows] if keep.all() else s[rows][:, keep]
        bad = margins(sub) <= MARGIN
        for r, p in copies:
            bad |= (rows == p) & (s[rows, r] >= sub.max(axis=1))
        bad &= ~np.isin(rows, list(fixed))
        if not bad.any():
            return s
        rows = rows[bad]
        zq[rows] = rs.randn(rows.size, zq.shape[1]).astype(F32)
        s[rows] = logits64(zq[rows], zk, w)
    raise AssertionError("no decided case found")


def _draw(rs, b, d, logit_scale):
    """logits of order logit_scale; the keys lean towards their own query's image, so that a share of the rows are hits"""
    zq = rs.randn(b, d).astype(F32)
    w = (rs.randn(d, d) * (logit_scale / d)).astype(F32)
    zk = (rs.randn(b, d) + zq.astype(F64) @ w.astype(F64)).astype(F32)
    return zq, zk, w


def hits(s):
    """rows whose FIRST arg-max is the diagonal"""
    return int((np.argmax(s, axis=1) == np.arange(s.shape[0])).sum())


@functools.lru_cache(maxsize=None)
def random_case(b, d, logit_scale=2.0):
    """-> (zq, zk, w, float64 logits)"""
    rs = np.random.RandomState(1000 * b + d + 1)
    zq, zk, w = _draw(rs, b, d, logit_scale)
    return zq, zk, w, settle(rs, zq, zk, w)


@functools.lru_cache(maxsize=None)
def planted_case(b, d):
    """Row PLANTED_ROW: the last key is 160 u / |u|^2 for u = zq W of that row -- a logit of 160 where every key of an
    earlier tile stays far below 60: the running sum is rescaled by exp(-100) or less, which is 0 in fp32.  Row b - 1 (b is
    one past a multiple of 32: the ragged last query tile, its diagonal in the last key tile) asks half the same question
    and is a hit."""
    assert b % TILE == 1 and b > TILE
    rs = np.random.RandomState(77 * b + d)
    zq, zk, w = _draw(rs, b, d, 2.0)
    u = zq[PLANTED_ROW].astype(F64) @ w.astype(F64)
    zk[b - 1] = (u * (160.0 / (u @ u))).astype(F32)
    zq[b - 1] = (0.5 * zq[PLANTED_ROW] + 0.05 * rs.randn(d)).astype(F32)
    return zq, zk, w, settle(rs, zq, zk, w, fixed=(PLANTED_ROW, b - 1))


@functools.lru_cache(maxsize=None)
def tie_case(b, d):
    """TIES planted: key r = 30 u / |u|^2 for u = zq W of row r (a logit of 30, the row's maximum by more than 1), key p
    its bitwise copy."""
    rs = np.random.RandomState(13 * b + d)
    zq, zk, w = _draw(rs, b, d, 2.0)
    for r, p in TIES:
        u = zq[r].astype(F64) @ w.astype(F64)
        zk[r] = (u * (30.0 / (u @ u))).astype(F32)
        zk[p] = zk[r]
    return zq, zk, w, settle(rs, zq, zk, w, fixed=[r for r, _ in TIES], copies=TIES)
