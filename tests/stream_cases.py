"""The streaming cases shared by tests/test_stream_host.py (which checks the oracle's own error on every prefix of every one of them)
and tests/test_gpu_stream.py (which streams them through csrc/track_stream.hip).  The oracle is tests/track_oracle.py, unchanged: the
value emitted for row g of a slot that holds the rows 0 .. f is track_oracle.smooth (or smooth_para) of those rows, read at row g."""
import numpy as np

import track_oracle as to

U = 2.0 ** -23
T_PLAIN = 70                                                   # every prefix length 1 .. 70; T = 1 .. 6 are where a stencil loses a term
WIDTHS = (1, 64, 65)                                           # both sides of a wave of 64 lanes
KINDS = ('ones', 'mid', 'first', 'rand')                       # all ones, a middle gap, only the first row observed, 40 % random zeros
LAGS = (0, 3, 70)                                              # lag 3: a ring of 8 rows wraps about 17 times over 70 rows (two flushes included)


def stream_conf(kind, T, rng):
    c = rng.uniform(0.2, 1.0, T).astype(np.float32)
    if kind == 'ones':
        c[:] = 1.0
    elif kind == 'mid':
        c[T // 3:(2 * T) // 3] = 0.0
    elif kind == 'first':
        c[1:] = 0.0
    elif kind == 'rand':
        c[1:][rng.uniform(size=T - 1) < 0.4] = 0.0
    return c


def plain_case(C, kind, T=T_PLAIN, seed=None):
    """-> (values [T,C] f32 with NaN in every row of weight 0, conf [T] f32); the first row is always observed."""
    rng = np.random.default_rng(1000 * C + KINDS.index(kind) if seed is None else seed)
    v = (rng.normal(0, 1, (T, C)) * rng.uniform(0.1, 3.0, C) + rng.normal(0, 2, C)).astype(np.float32)
    c = stream_conf(kind, T, rng)
    v[c == 0] = np.nan
    return v, c


_PLAIN = {}


def plain_refs(C, kind, lam):
    """Per prefix length f + 1: (the banded oracle's x [f+1,C] float64, the bound's two terms: max |x| and the two-solver gap)."""
    key = (C, kind, tuple(lam))
    if key not in _PLAIN:
        v, c = plain_case(C, kind)
        refs = []
        for f in range(len(c)):
            b = to.solve_banded(v[:f + 1], c[:f + 1], lam[0], lam[1])
            d = to.solve_dense(v[:f + 1], c[:f + 1], lam[0], lam[1])
            refs.append((b, float(np.abs(b).max()), float(np.abs(b - d).max()), float(np.abs(d).max())))
        _PLAIN[key] = refs
    return _PLAIN[key]


def para_tracks():
    """The recovery case's three tracks plus the T = 1 and T = 2 tracks of track_oracle.para_case(): a list of (para [T,229] f32 with
    NaN gap rows, conf [T] f32), and the recovery case's dict."""
    para, conf, start, rc = to.para_case()
    return [(para[start[k]:start[k + 1]], conf[start[k]:start[k + 1]]) for k in range(5)], rc


_PARA = {}


def para_refs(shared):
    """Per track and prefix length: (banded smooth_para dict, |banded - dense| of 'ch' [f+1,157])."""
    if shared not in _PARA:
        out = []
        for para, conf in para_tracks()[0]:
            per = []
            for f in range(len(conf)):
                ts = np.array([0, f + 1])
                b = to.smooth_para(para[:f + 1], conf[:f + 1], ts, to.DEFAULT_LAM, shared)
                d = to.smooth_para(para[:f + 1], conf[:f + 1], ts, to.DEFAULT_LAM, shared, solver=to.solve_dense)
                per.append((b, np.abs(b['ch'] - d['ch']), d['ch']))
            out.append(per)
        _PARA[shared] = out
    return _PARA[shared]


def para_ratio(got, ref, gap, g):
    """One emitted [229] row against the oracle on its prefix: -> {'cam', 'betas', 'rot'} measured / bound (the bounds of
    tests/test_gpu_tracks.py: 8 x 2^-23 x max |f64| of the block plus four times the two-solver difference; rotations four times the
    float32 oracle's error plus 8 roundings of 1)."""
    r = {}
    for name, sl in (('cam', slice(0, 3)), ('betas', slice(3, 13))):
        bound = 8 * U * np.abs(ref['para64'][:, sl]).max() + 4 * gap[:, sl].max()
        r[name] = np.abs(got[sl] - ref['para64'][g, sl]).max() / bound
    err32 = np.abs(ref['para32'][:, 13:].astype(np.float64) - ref['para64'][:, 13:]).max()
    r['rot'] = np.abs(got[13:] - ref['para64'][g, 13:]).max() / (4 * err32 + 8 * U)
    return r
