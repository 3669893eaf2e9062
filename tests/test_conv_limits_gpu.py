"""The contraction kernels (csrc/mfma_conv.hip, mfma_dispatch.h, mfma_igemm.h, mfma_wgrad.h, mfma_generic.h, mfma_pair.h,
img_conv.hip) at every arm of their dispatchers, against tests/conv_ref.py -- the plain float64 restatement of the three
operations -- on float64 copies of the fp32 inputs.

Every case names, per route, the launch it must produce (arl_dev_conv_launch_log: kernel family, tile, flags, grid, split
count), so that no case silently runs another kernel than the one it was written for; the shapes are the smallest that
reach each arm.  Inputs are those of tests/test_mfma_conv_gpu.py (randn, 30 % exact zeros in x, weights scaled by
1 / sqrt(kh kw C)).  Bounds (the project's own):
  * routes SPLIT9 / SPLIT6 / FP32 and the generic kernels: max|got - want| <= 2e-5 sqrt(K_red) max(max|want|, 1e-6), K_red =
    kh kw C (forward), taps * K (data gradient), b Ho Wo (weight / bias gradient);
  * outputs of >= 1 024 elements: relative rms <= 6e-7, a split route <= 1.5 x the FP32 route's on the same inputs + 3e-8;
  * route BF16: the first bound against conv_ref on rounded() operands -- the unrounded ones where the log shows an
    fp32-chain kernel (<= 16 columns, generic kernels), as tests/test_bf16_route_gpu.py documents;
  * bit for bit: run to run, across tile choices (arl_dev_fwd_tile), data gradient on k-contiguous against gathered
    weights, arl_conv2d_bwd_pair against the separate calls (but for the split reduction the existing test allows).
Outputs are pre-filled with NaN and must come out finite; input pixels no window reads get a data gradient of exactly 0.
Each test prints its error / bound ratios (pytest -s)."""
import collections

import numpy as np
import pytest
import torch

import conv_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

L = collections.namedtuple("L", "family tile flags grid splits minw")


def launch(family, tile, flags="", grid=(1, 1, 1), splits=1, minw=0):
    return L(family, tuple(tile), frozenset(flags.split()), tuple(grid), splits, minw)


def fold(splits, total):
    """The fold of `splits` partial sums of `total` floats: 16 threads per output float4 and 64 outputs per block, or 64
    threads and 16 outputs from 128 splits on (the wide fold)."""
    wide = splits >= 128
    return launch("fold", (64 if wide else 16, 0, 0, 0, 0), "", (-(-(total // 4) // (16 if wide else 64)), 1, 1), splits)


def plan_split(tiles, red, want):
    """csrc/mfma_dispatch.h plan_split: (splits, rows per split) so that tiles * splits ~ want, >= 4 k-tiles of 32 per split."""
    s = 1 if tiles >= want else want // tiles
    s = max(1, min(s, (red + 127) // 128))
    per = -(-(-(-red // s)) // 32) * 32
    return -(-red // per), per


# the launcher instantiations (tile, flags that are template arguments, minw) the cases below name
IG16 = dict(family="igemm", tile=(4, 1, 2, 1, 16))                       # launch_igemm<4,1,2,1,16,*,N16>
SP411 = dict(family="igemm_split", tile=(4, 1, 1, 1, 32), minw=2)
SP412 = dict(family="igemm_split", tile=(4, 1, 1, 2, 32), minw=2)
SP2211 = dict(family="igemm_split", tile=(2, 2, 1, 1, 32), minw=3)
SP2222 = dict(family="igemm_split", tile=(2, 2, 2, 2, 32), minw=1)
OCC14 = dict(family="igemm_occ", tile=(1, 4, 2, 1, 32), minw=5)           # launch_n64 / small32
OCC22 = dict(family="igemm_occ", tile=(2, 2, 2, 1, 32), minw=5)
RG41 = dict(family="rowgather", tile=(4, 1, 2, 1, 16))
RG2221 = dict(family="rowgather", tile=(2, 2, 2, 1, 16))
RG2211 = dict(family="rowgather", tile=(2, 2, 1, 1, 16))
RG2222 = dict(family="rowgather", tile=(2, 2, 2, 2, 16))

ROUTES = ("split9", "split6", "fp32", "bf16")
SPLIT_ROUTES = ("split9", "split6", "bf16")
# kernels that multiply bf16 pieces: on route BF16 their operands are rounded; every other family is an fp32 chain
PIECE_FAMILIES = ("igemm_split", "wgrad_split", "bwd_pair", "conv1_img")
FIGURES = collections.defaultdict(float)          # (op, route) -> largest error / bound seen (printed by every test)


def _route(name):
    from accel_rl_amd import _lib
    return dict(split9=_lib.ROUTE_SPLIT9, split6=_lib.ROUTE_SPLIT6, fp32=_lib.ROUTE_FP32, bf16=_lib.ROUTE_BF16)[name]


def _geom(row, route):
    from accel_rl_amd import _lib
    return _lib.conv_geom(*row, route=_route(route))


def _inputs(row, seed=0):
    b, H, W, C, K, kh, kw, st, ph, pw = row
    ho, wo = conv_ref.out_hw(row)
    gen = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn(b, H, W, C, device=DEV, generator=gen)
    x = torch.where(torch.rand(x.shape, device=DEV, generator=gen) < 0.3, torch.zeros_like(x), x)
    w = torch.randn(K, kh, kw, C, device=DEV, generator=gen) / np.sqrt(kh * kw * C)
    bias = torch.randn(K, device=DEV, generator=gen)
    dy = torch.randn(b, ho, wo, K, device=DEV, generator=gen)
    mask = torch.randn(b, H, W, C, device=DEV, generator=gen)
    mask.view(-1)[0::7] = 0.0                       # the mask rule is mask > 0: both zeros (and negatives) zero the element
    mask.view(-1)[3::7] = -0.0
    return x, w, bias, dy, mask


def _tol(want, k_red):
    return 2e-5 * np.sqrt(k_red) * max(want.abs().max().item(), 1e-6)


def _rel_rms(got, want):
    return ((got.double() - want).pow(2).mean().sqrt() / want.pow(2).mean().sqrt()).item()


def _nan(*shape):
    return torch.full(shape, float("nan"), device=DEV)


SEEN = set()           # every launcher instantiation a launch log of this session showed (the census compares)
RAN = set()            # the dispatch-arm cases that ran to their end


def _instantiation(l):
    """(family, tile, the flags that are template arguments of the launcher: b_kc / u8 / n16, minw)"""
    plain = l.family in ("igemm", "wgrad_fast", "bwd_pair")
    return (l.family, l.tile, frozenset() if l.family == "bwd_pair" else l.flags & {"b_kc", "u8", "n16"}, 0 if plain else l.minw)


def _log():
    from accel_rl_amd import _lib
    got = _lib.conv_launch_log()
    SEEN.update(_instantiation(l) for l in got)
    return got


def _same_launch(got, want, ctx):
    assert (got.family, got.tile, got.flags, got.grid, got.splits) == (want.family, want.tile, want.flags, want.grid, want.splits), \
        (ctx, got, want)
    assert not want.minw or got.minw == want.minw, (ctx, got, want)


def _check_log(want, ctx, split_mode, got=None):
    """The whole log of the last call (or the log `got`, read earlier) is the list `want`, and carries the route's split mode."""
    got = _log() if got is None else got
    assert len(got) == len(want), (ctx, got, want)
    for g, w_ in zip(got, want):
        _same_launch(g, w_, ctx)
        assert g.split_mode == split_mode, (ctx, g)
    return got


SPLIT_MODE = dict(split9=9, split6=6, fp32=0, bf16=1)


class Errors(object):
    """Per case: max-error / bound per (op, run), the rms figures, and the bars between routes."""

    def __init__(self, case):
        self.case, self.rms = case, {}

    def check(self, op, run, got, want, k_red, rms=True):
        assert torch.isfinite(got).all(), (self.case, op, run)
        err, tol = (got.double() - want).abs().max().item(), _tol(want, k_red)
        route = run.split("/")[0]
        FIGURES[op, route] = max(FIGURES[op, route], err / tol)
        print("%s %s %s: max err %.3g = %.3f of the bound" % (self.case, op, run, err, err / tol))
        assert err <= tol, (self.case, op, run, err, tol)
        if rms and got.numel() >= 1024 and not run.startswith("bf16") and want.abs().max().item() > 0:
            self.rms[op, run] = _rel_rms(got, want)
            print("%s %s %s: rel rms %.3g" % (self.case, op, run, self.rms[op, run]))
            assert self.rms[op, run] <= 6e-7, (self.case, op, run, self.rms[op, run])

    def split_routes_against_fp32(self):
        for (op, run), e in self.rms.items():
            route, _, rest = run.partition("/")
            if route in ("split9", "split6") and (op, "fp32/" + rest if rest else "fp32") in self.rms:
                e0 = self.rms[op, "fp32/" + rest if rest else "fp32"]
                assert e <= 1.5 * e0 + 3e-8, (self.case, op, run, e, e0)


@pytest.fixture(autouse=True)
def _hooks_off():
    from accel_rl_amd import _lib
    lib = _lib.load()
    yield
    lib.arl_dev_conv_force_generic(0)
    lib.arl_dev_fwd_tile(-1)
    lib.arl_dev_conv_variant(0)
    lib.arl_dev_dgrad_wt(1)
    print("largest error / bound so far:", {"%s %s" % k: round(v, 3) for k, v in sorted(FIGURES.items())})


# ------------------------------------------------------------------------------------------------------------------
# forward
# ------------------------------------------------------------------------------------------------------------------
def _fwd_case(row, split, fp32, generic=None, tiles=(), note=""):
    """split / fp32 / generic: the launches of the bf16-split routes (SPLIT9, SPLIT6, BF16 run one kernel family), of route
    FP32, and under arl_dev_conv_force_generic (None: not run forced); tiles: arl_dev_fwd_tile values that must give the
    same bits on the split routes."""
    as_list = lambda v: None if v is None else (list(v) if isinstance(v, (list, tuple)) and not isinstance(v, L) else [v])  # noqa: E731
    return dict(row=row, split=as_list(split), fp32=as_list(fp32), generic=as_list(generic), tiles=tiles, note=note)


def _n16(row, grid, flags="", generic_grid=(1, 1, 1)):
    """<= 16 output columns: launch_igemm<4,1,2,1,16,true,N16> on every route (128-row tiles of 16-wide MFMAs)."""
    l = launch(flags="b_kc n16 " + flags, grid=grid, **IG16)
    return _fwd_case(row, l, l, None if generic_grid is None else launch(flags="b_kc", grid=generic_grid, **RG41))


FWD = [
    # ---- fast path
    _n16((3, 5, 5, 32, 4, 1, 1, 1, 0, 0), (1, 1, 1)),               # N = 4: 75 rows on a 128-row tile
    _n16((3, 5, 5, 32, 12, 1, 1, 1, 0, 0), (1, 1, 1)),
    _n16((3, 5, 5, 32, 16, 1, 1, 1, 0, 0), (1, 1, 1)),
    _n16((2, 12, 16, 4, 12, 8, 8, 4, 0, 0), (1, 1, 1), "multi_tap"),   # C = 4, kw = 8: eight taps per k-tile, M = 12
    _n16((5, 6, 5, 16, 16, 2, 2, 1, 1, 1), (2, 1, 1), "multi_tap has_pad"),      # 210 rows
    # N = 20, ragged columns; 168 rows: the second row tile holds 40
    _fwd_case((4, 7, 6, 32, 20, 3, 3, 1, 1, 1), launch(flags="b_kc has_pad direct", grid=(2, 1, 1), **SP411),
              launch("igemm", (4, 1, 1, 1, 16), "b_kc has_pad", (2, 1, 1)), launch(flags="b_kc", **RG41)),
    # N = 36: the column split (v == 1), the second column tile holds 4 columns; FP32: launch_n64
    _fwd_case((4, 7, 6, 32, 36, 3, 3, 1, 1, 1), launch(flags="b_kc has_pad direct", grid=(2, 2, 1), **SP411),
              launch(flags="b_kc has_pad n16", grid=(6, 1, 1), **OCC14), launch(flags="b_kc", grid=(2, 1, 1), **RG2221),
              tiles=(0, 2)),
    # 129 row tiles: 128 x 64 tiles (v == 0) by size; 16 rows in the last tile
    _fwd_case((16400, 1, 1, 32, 36, 1, 1, 1, 0, 0), launch(flags="b_kc direct", grid=(129, 1, 1), **SP412),
              launch(flags="b_kc n16", grid=(513, 1, 1), **OCC14), launch(flags="b_kc", grid=(129, 1, 1), **RG2221)),
    # `small`: 2 splits of 96 and 64; three column tiles, the last of 4 columns; the fold applies bias and rectifier
    _fwd_case((5, 1, 1, 160, 132, 1, 1, 1, 0, 0), [launch(flags="b_kc", grid=(1, 3, 2), splits=2, **SP2211), fold(2, 660)],
              [launch(flags="b_kc n16", grid=(1, 3, 2), splits=2, **OCC14), fold(2, 660)],
              [launch(flags="b_kc", grid=(1, 3, 2), splits=2, **RG2211), fold(2, 660)]),
    # 128 and 127 splits, either side of the wide fold; M = 1
    _fwd_case((1, 1, 1, 16384, 128, 1, 1, 1, 0, 0), [launch(flags="b_kc", grid=(1, 2, 128), splits=128, **SP2211), fold(128, 128)],
              [launch(flags="b_kc n16", grid=(1, 2, 128), splits=128, **OCC14), fold(128, 128)],
              [launch(flags="b_kc", grid=(1, 2, 128), splits=128, **RG2211), fold(128, 128)]),
    _fwd_case((1, 1, 1, 16256, 128, 1, 1, 1, 0, 0), [launch(flags="b_kc", grid=(1, 2, 127), splits=127, **SP2211), fold(127, 128)],
              [launch(flags="b_kc n16", grid=(1, 2, 127), splits=127, **OCC14), fold(127, 128)],
              [launch(flags="b_kc", grid=(1, 2, 127), splits=127, **RG2211), fold(127, 128)]),
    # not small: 99 tiles of 128 x 128 with 2 splits, ragged in both dimensions
    _fwd_case((4100, 1, 1, 256, 260, 1, 1, 1, 0, 0),
              [launch(flags="b_kc", grid=(33, 3, 2), splits=2, **SP2222), fold(2, 4100 * 260)],
              [launch("igemm", (2, 2, 2, 2, 32), "b_kc", (33, 3, 2), 2), fold(2, 4100 * 260)],
              [launch(flags="b_kc", grid=(33, 3, 2), splits=2, **RG2222), fold(2, 4100 * 260)]),
    # fill64: 130 tiles of 128 x 128 fill 51 % of the CUs, 387 of 64 x 64 fill 76 %
    _fwd_case((8200, 1, 1, 32, 132, 1, 1, 1, 0, 0), launch(flags="b_kc", grid=(129, 3, 1), **SP2211),
              launch("igemm", (2, 2, 2, 2, 32), "b_kc", (65, 2, 1)), launch(flags="b_kc", grid=(65, 2, 1), **RG2222)),
    # 256 tiles of 128 x 128 fill the CUs: the 64 x 64 tiles must not be chosen
    _fwd_case((16260, 1, 1, 32, 132, 1, 1, 1, 0, 0), launch(flags="b_kc", grid=(128, 2, 1), **SP2222),
              launch("igemm", (2, 2, 2, 2, 32), "b_kc", (128, 2, 1)), launch(flags="b_kc", grid=(128, 2, 1), **RG2222)),
    # 2^21 rows of 2048 output columns: (rows + 256) * 2048 >= 2^32, both magic multipliers 0 (real division) ...
    _n16((1024, 1, 2055, 4, 4, 1, 8, 1, 0, 0), (16384, 1, 1), "multi_tap", None),
    # ... and the largest row count the magic division is valid for
    _n16((1023, 1, 2055, 4, 4, 1, 8, 1, 0, 0), (16368, 1, 1), "multi_tap", None),
    # padding >= kernel: whole windows in the border, outputs = bias (rectified) exactly
    _n16((2, 3, 3, 32, 8, 2, 2, 1, 2, 2), (1, 1, 1), "has_pad"),
    _n16((1, 3, 4, 32, 8, 3, 4, 1, 0, 0), (1, 1, 1)),               # M = 1: a single output pixel, batch 1
    # non-square kernel, asymmetric padding, rows the stride never reaches
    _fwd_case((3, 9, 7, 32, 20, 3, 2, 2, 1, 0), launch(flags="b_kc has_pad direct", **SP411),
              launch("igemm", (4, 1, 1, 1, 16), "b_kc has_pad"), launch(flags="b_kc", **RG41)),
    # ---- generic by shape (C = 12: no k-tile of 32 inside a filter row; 49 taps with padding)
    _fwd_case((4, 7, 6, 12, 20, 3, 3, 1, 1, 1), launch(flags="b_kc", **RG41), launch(flags="b_kc", **RG41)),
    _fwd_case((4, 7, 6, 12, 36, 3, 3, 1, 1, 1), launch(flags="b_kc", grid=(2, 1, 1), **RG2221),
              launch(flags="b_kc", grid=(2, 1, 1), **RG2221)),
    _fwd_case((4, 7, 6, 12, 68, 3, 3, 1, 1, 1), launch(flags="b_kc", grid=(2, 1, 1), **RG2222),
              launch(flags="b_kc", grid=(2, 1, 1), **RG2222)),
    # generic split-K: 2 splits of 96 and 36
    _fwd_case((5, 1, 1, 132, 132, 1, 1, 1, 0, 0), [launch(flags="b_kc", grid=(1, 3, 2), splits=2, **RG2211), fold(2, 660)],
              [launch(flags="b_kc", grid=(1, 3, 2), splits=2, **RG2211), fold(2, 660)]),
    _fwd_case((8200, 1, 1, 12, 132, 1, 1, 1, 0, 0), launch(flags="b_kc", grid=(65, 2, 1), **RG2222),
              launch(flags="b_kc", grid=(65, 2, 1), **RG2222)),
    _fwd_case((2, 9, 8, 32, 8, 7, 7, 1, 3, 3), launch(flags="b_kc", **RG41), launch(flags="b_kc", **RG41)),
]
# the two 2^21-row cases run their forced-generic pass once (route SPLIT9 only, inside the case: generic_grid=None above
# skips it there); it is this case
FWD_GENERIC_ONCE = ((1024, 1, 2055, 4, 4, 1, 8, 1, 0, 0), launch(flags="b_kc", grid=(8192, 1, 1), **RG41))


def _ids(cases):
    return ["x".join(str(v) for v in c["row"]) for c in cases]


def _fwd_refs(row, x, w, bias):
    """(bias + relu, no bias no relu) float64 references, for the operands as they are and rounded to bf16."""
    refs = {}
    for rounded in (False, True):
        xs, ws = (conv_ref.rounded(x), conv_ref.rounded(w)) if rounded else (x, w)
        bare = conv_ref.fwd(xs, ws, None, row, False)
        refs[rounded] = ((bare + bias.double()).clamp(min=0), bare)
    return refs


def _run_fwd(row, route, x, w, bias, ws, relu):
    from accel_rl_amd import _lib
    b, H, W, C, K = row[:5]
    ho, wo = conv_ref.out_hw(row)
    y = _nan(b, ho, wo, K)
    _lib.conv2d_fwd(x, w, bias if relu else None, y, _geom(row, route), relu, ws)
    return y


@pytest.mark.parametrize("case", FWD, ids=_ids(FWD))
def test_forward_at_every_dispatch_arm(case):
    from accel_rl_amd import _lib
    lib = _lib.load()
    row = case["row"]
    b, H, W, C, K, kh, kw, st, ph, pw = row
    x, w, bias, _, _ = _inputs(row)
    ws = _lib.conv_workspace(DEV)
    refs = _fwd_refs(row, x, w, bias)
    # windows wholly in the padded border (none of their taps meets the image): the output is the bias, exactly
    border = conv_ref.fwd(torch.ones_like(x), torch.ones_like(w), None, row, False) == 0
    errs = Errors(row)
    runs = [(r, False) for r in ROUTES] + ([(r, True) for r in ROUTES] if case["generic"] else [])
    for route, forced in runs:
        lib.arl_dev_conv_force_generic(int(forced))
        name = route + ("/generic" if forced else "")
        want_log = case["generic"] if forced else case["fp32" if route == "fp32" else "split"]
        for relu in (True, False):
            y = _run_fwd(row, route, x, w, bias, ws, relu)
            got_log = _check_log(want_log, (row, name), SPLIT_MODE[route])
            rounded = route == "bf16" and got_log[0].family in PIECE_FAMILIES
            errs.check("fwd", name + ("/relu" if relu else ""), y, refs[rounded][0 if relu else 1], kh * kw * C)
            assert torch.equal(y, _run_fwd(row, route, x, w, bias, ws, relu)), (row, name, "second run")
            if relu and border.any():
                assert torch.equal(y[border], bias.clamp(min=0).expand_as(y)[border]), (row, name, "border windows")
        lib.arl_dev_conv_force_generic(0)
        if not forced and route != "fp32":
            y = _run_fwd(row, route, x, w, bias, ws, True)
            for v in case["tiles"]:                     # other tile shapes: another launch, the same bits
                lib.arl_dev_fwd_tile(v)
                yv = _run_fwd(row, route, x, w, bias, ws, True)
                lib.arl_dev_fwd_tile(-1)
                assert _log()[0].tile != case["split"][0].tile and torch.equal(y, yv), (row, route, v)
    errs.split_routes_against_fp32()
    RAN.add(("fwd", row))


def test_forward_generic_kernel_at_two_million_rows():
    """The forced-generic pass of the 2^21-row shape (the fast kernels' passes: the FWD cases), run once."""
    from accel_rl_amd import _lib
    lib = _lib.load()
    row, want_log = FWD_GENERIC_ONCE
    x, w, bias, _, _ = _inputs(row)
    ws = _lib.conv_workspace(DEV)
    want = (conv_ref.fwd(x, w, None, row, False) + bias.double()).clamp(min=0)
    lib.arl_dev_conv_force_generic(1)
    y = _run_fwd(row, "split9", x, w, bias, ws, True)
    _check_log([want_log], row, 9)
    Errors(row).check("fwd", "split9/generic/relu", y, want, row[5] * row[6] * row[3])


# ------------------------------------------------------------------------------------------------------------------
# data gradient
# ------------------------------------------------------------------------------------------------------------------
def _dg_case(row, split, fp32, generic=None, wt=None, pair_split=None, pair_fp32=None, tiles=(), classes=1, paired=False):
    """split / fp32 / generic as in the forward; wt: the split routes' launch on k-contiguous weights (None: the same launch);
    pair_*: the data-gradient launches of arl_conv2d_bwd_pair where they differ from the bare call's (a split reduction);
    classes: launches of a generic data gradient (one per input-pixel parity class)."""
    as_list = lambda v: None if v is None else (list(v) if isinstance(v, list) else [v])      # noqa: E731
    return dict(row=row, split=as_list(split), fp32=as_list(fp32), generic=as_list(generic), wt=as_list(wt),
                pair_split=as_list(pair_split), pair_fp32=as_list(pair_fp32), tiles=tiles, classes=classes, paired=paired)


def _dg16(row, grid, flags="has_pad", classes=1, gen=RG41):
    """<= 16 input channels: launch_igemm<4,1,2,1,16,false,N16> on every route."""
    l = launch(flags="n16 " + flags, grid=grid, **IG16)
    return _dg_case(row, l, l, launch(flags="tap_uniform", **gen), classes=classes)


DGRAD = [
    _dg16((3, 5, 5, 16, 32, 3, 3, 1, 1, 1), (1, 1, 1)),
    _dg16((3, 5, 5, 4, 32, 3, 3, 1, 1, 1), (1, 1, 1)),
    # odd image: four parity classes of 12, 8, 9 and 6 pixels
    _dg16((3, 7, 5, 8, 32, 4, 4, 2, 1, 1), (1, 1, 4), classes=4),
    # C = 20: 17 .. 32 columns
    _dg_case((3, 7, 5, 20, 32, 4, 4, 2, 1, 1), launch(flags="has_pad direct", grid=(1, 1, 4), **SP411),
             launch(flags="has_pad n16", grid=(1, 1, 4), **OCC22), launch(flags="tap_uniform", **RG41),
             wt=launch(flags="b_kc has_pad direct", grid=(1, 1, 4), **SP411), classes=4),
    # C = 36: the column split by size; tile hooks 0 and 1 give the same bits; FP32: launch_n64<false>
    _dg_case((3, 7, 5, 36, 32, 4, 4, 2, 1, 1), launch(flags="has_pad direct", grid=(1, 2, 4), **SP411),
             launch(flags="has_pad n16", grid=(2, 1, 4), **OCC14), launch(flags="tap_uniform", **RG2221),
             wt=launch(flags="b_kc has_pad direct", grid=(1, 2, 4), **SP411), tiles=(0, 1), classes=4),
    # 4 classes x 35 row tiles = 140 tiles: 128 x 64 tiles by size (2 x 2 kernel, stride 2: one tap per class)
    _dg_case((70, 16, 16, 36, 32, 2, 2, 2, 0, 0), launch(flags="has_pad direct", grid=(35, 1, 4), **SP412),
             launch(flags="has_pad n16", grid=(140, 1, 4), **OCC14), launch(flags="tap_uniform", grid=(35, 1, 1), **RG2221),
             wt=launch(flags="b_kc has_pad direct", grid=(35, 1, 4), **SP412), classes=4),
    # 68 columns on 128 x 128 tiles
    _dg_case((3, 7, 5, 68, 32, 4, 4, 2, 1, 1), launch(flags="has_pad", grid=(1, 1, 4), **SP2222),
             launch("igemm", (2, 2, 2, 2, 32), "has_pad", (1, 1, 4)), launch(flags="tap_uniform", **RG2222), classes=4),
    # `small`: one split through the bare call (it has no workspace), 2 splits and a masked fold through the pair call
    _dg_case((5, 1, 1, 132, 160, 1, 1, 1, 0, 0), launch(grid=(1, 3, 1), **SP2211),
             launch("igemm", (2, 2, 1, 1, 32), "", (1, 3, 1)), launch(flags="tap_uniform", grid=(1, 2, 1), **RG2222),
             pair_split=[launch(grid=(1, 3, 2), splits=2, **SP2211), fold(2, 660)],
             pair_fp32=[launch("igemm", (2, 2, 1, 1, 32), "", (1, 3, 2), 2), fold(2, 660)]),
    # 32 taps (non-square 8 x 4) stay on the fast path, 36 taps leave it
    _dg_case((2, 9, 9, 32, 32, 8, 4, 1, 1, 1), launch(flags="has_pad direct", grid=(2, 1, 1), **SP411),
             launch(flags="has_pad n16", grid=(3, 1, 1), **OCC22), launch(flags="tap_uniform", **RG41),
             wt=launch(flags="b_kc has_pad direct", grid=(2, 1, 1), **SP411)),
    _dg_case((2, 9, 9, 32, 32, 6, 6, 1, 1, 1), launch(flags="tap_uniform", **RG41), launch(flags="tap_uniform", **RG41)),
    # stride 4 and 3: generic, 16 and 9 parity classes
    _dg_case((2, 12, 16, 4, 32, 8, 8, 4, 0, 0), launch(flags="tap_uniform", **RG41), launch(flags="tap_uniform", **RG41),
             classes=16),
    _dg_case((2, 7, 8, 8, 32, 3, 3, 3, 0, 0), launch(flags="tap_uniform", **RG41), launch(flags="tap_uniform", **RG41),
             classes=9),
    # H < stride: two classes only; column 4 is never read
    _dg16((2, 1, 5, 8, 32, 2, 2, 2, 1, 0), (1, 1, 2), classes=2),
    # generic by K: uniform taps (K = 16, 48: a 16-wide k-tile stays inside one tap) and straddling ones (K = 20)
    _dg_case((3, 7, 5, 20, 16, 4, 4, 2, 1, 1), launch(flags="tap_uniform", **RG41), launch(flags="tap_uniform", **RG41),
             classes=4),
    _dg_case((3, 7, 5, 36, 48, 4, 4, 2, 1, 1), launch(flags="tap_uniform", **RG2221),
             launch(flags="tap_uniform", **RG2221), classes=4),
    _dg_case((3, 7, 5, 68, 20, 4, 4, 2, 1, 1), launch(**RG2222), launch(**RG2222), classes=4),
    # both gradients of a wide layer in one launch (the one shape here that pairs; 6 x 16 = 96 output pixels)
    _dg_case((16, 7, 5, 68, 96, 4, 4, 2, 1, 1), launch(flags="has_pad", grid=(2, 1, 4), **SP2222),
             launch("igemm", (2, 2, 2, 2, 32), "has_pad", (2, 1, 4)),
             pair_split=[launch("bwd_pair", (2, 2, 2, 2, 16), "has_pad", (8 + 9, 1, 1))],
             pair_fp32=[launch("bwd_pair", (2, 2, 2, 2, 32), "has_pad", (8 + 9, 1, 1))], classes=4, paired=True),
]


def _dg_refs(row, dy, w, mask):
    return {r: (conv_ref.dgrad(a, c, row), conv_ref.dgrad(a, c, row, mask))
            for r, (a, c) in ((False, (dy, w)), (True, (conv_ref.rounded(dy), conv_ref.rounded(w))))}


@pytest.mark.parametrize("case", DGRAD, ids=_ids(DGRAD))
def test_data_gradient_at_every_dispatch_arm(case):
    from accel_rl_amd import _lib
    lib = _lib.load()
    row = case["row"]
    b, H, W, C, K, kh, kw, st, ph, pw = row
    x, w, _, dy, mask = _inputs(row, seed=1)
    k_red = (kh // st) * (kw // st) * K
    refs = _dg_refs(row, dy, w, mask)
    want_dw = {r: conv_ref.wgrad(*((conv_ref.rounded(dy), conv_ref.rounded(x)) if r else (dy, x)), row) for r in (False, True)}
    unread = ~conv_ref.reads(row).to(DEV)
    errs = Errors(row)
    use_wt = 16 < C <= 64 and st <= 2 and H >= st and W >= st
    runs = [(r, False) for r in ROUTES] + ([(r, True) for r in ROUTES] if case["generic"] else [])
    for route, forced in runs:
        lib.arl_dev_conv_force_generic(int(forced))
        name = route + ("/generic" if forced else "")
        geom = _geom(row, route)
        key = "fp32" if route == "fp32" else "split"
        want_log = case["generic"] if forced else case[key]
        repeat = case["classes"] if want_log[0].family == "rowgather" else 1
        dxs = {}
        for m in (None, mask):
            tag = name + ("/masked" if m is not None else "")
            dx = _nan(b, H, W, C)
            _lib.conv2d_bwd_data(dy, w, m, dx, geom)
            got_log = _log()
            if repeat > 1:                              # one launch per parity class: the same kernel, its own grid
                assert len(got_log) == repeat and all((g.family, g.tile, g.flags) == (want_log[0].family, want_log[0].tile,
                                                       want_log[0].flags) for g in got_log), (row, tag, got_log)
            else:
                _check_log(want_log, (row, tag), SPLIT_MODE[route])
            rounded = route == "bf16" and got_log[0].family in PIECE_FAMILIES
            errs.check("dgrad", tag, dx, refs[rounded][0 if m is None else 1], k_red)
            assert (dx[:, unread] == 0).all(), (row, tag, "pixels no window reads")
            dx2 = _nan(b, H, W, C)
            _lib.conv2d_bwd_data(dy, w, m, dx2, geom)
            assert torch.equal(dx, dx2), (row, tag, "second run")
            dxs[m is not None] = dx
        assert torch.equal(dxs[True], torch.where(mask > 0, dxs[False], torch.zeros_like(dxs[False]))), (row, name, "mask rule")
        # ---- on the k-contiguous copy of the weights: the same bits
        wk = None
        if use_wt:
            wk = _nan(w.numel())
            _lib.conv2d_dgrad_weights([(w, wk, geom)])
            assert [g.family for g in _log()] == ["dgrad_weights"]
            for m in (None, mask):
                dx = _nan(b, H, W, C)
                _lib.conv2d_bwd_data(dy, w, m, dx, geom, wt=wk)
                if route != "fp32" and not forced and want_log[0].family == "igemm_split":
                    _check_log(case["wt"], (row, name, "wt"), SPLIT_MODE[route])
                assert torch.equal(dx, dxs[m is not None]), (row, name, "k-contiguous weights")
        # ---- other tile shapes: another launch, the same bits
        if not forced and route != "fp32":
            for v in case["tiles"]:
                for wt_ in ((None, wk) if use_wt else (None,)):
                    lib.arl_dev_fwd_tile(v)
                    dx = _nan(b, H, W, C)
                    _lib.conv2d_bwd_data(dy, w, mask, dx, geom, wt=wt_)
                    lib.arl_dev_fwd_tile(-1)
                    assert _log()[0].family == "igemm_split" and torch.equal(dx, dxs[True]), (row, route, v)
            if case["tiles"]:
                lib.arl_dev_fwd_tile(0)
                _lib.conv2d_bwd_data(dy, w, mask, _nan(b, H, W, C), geom)
                lib.arl_dev_fwd_tile(-1)
                assert _log()[0].tile == SP412["tile"]
        # ---- through arl_conv2d_bwd_pair: bit-equal to the separate calls, but for the documented split reduction
        dw0 = _nan(K, kh, kw, C)
        wsp = _lib.conv_workspace(DEV)
        _lib.conv2d_bwd_weight(dy, x, dw0, geom, wsp)
        wfam = _log()[0].family
        wgrad_fast = wfam in ("wgrad_fast", "wgrad_split")
        split_ok = st == 1 and C > 64 and x.numel() <= 1 << 20
        for m in (None, mask):
            tag = name + "/pair" + ("/masked" if m is not None else "")
            dx, dw, db = _nan(b, H, W, C), _nan(K, kh, kw, C), _nan(K)
            folds = _lib.FoldList()
            done = folds.conv2d_bwd_pair(dy, w, m, dx, x, dw, geom, wsp, dbias=db, wt=wk)
            got_log = _log()
            folds.run()
            want_pair = None if forced else case["pair_fp32" if route == "fp32" else "pair_split"]
            if case["paired"] and not forced:
                _check_log(want_pair, (row, tag), SPLIT_MODE[route], got_log)
            elif want_pair:
                for g, w_ in zip(got_log, want_pair):
                    _same_launch(g, w_, (row, tag))
                assert len(got_log) == len(want_pair) + 1
            else:
                assert got_log[0].family == want_log[0].family and got_log[0].tile == want_log[0].tile, (row, tag, got_log)
            assert done == wgrad_fast and torch.equal(dw, dw0), (row, tag, "dw of the pair call")
            same = torch.equal(dx, dxs[m is not None])
            rounded = route == "bf16" and got_log[0].family in PIECE_FAMILIES
            if not same:
                assert split_ok and want_pair, (row, tag, "dx of the pair call")
                errs.check("dgrad", tag, dx, refs[rounded][0 if m is None else 1], k_red)
                assert (dx - dxs[m is not None]).abs().max().item() <= 2e-6 * np.sqrt(dy.numel() / b) * dx.abs().max().item()
            if done:
                errs.check("dbias", tag, db, conv_ref.dbias(dy), b * dy.shape[1] * dy.shape[2], rms=False)
            else:
                assert torch.isnan(db).all()
        rounded_w = route == "bf16" and wfam in PIECE_FAMILIES
        errs.check("wgrad", name + "/of the dgrad case", dw0, want_dw[rounded_w], b * dy.shape[1] * dy.shape[2])
        lib.arl_dev_conv_force_generic(0)
    errs.split_routes_against_fp32()
    RAN.add(("dgrad", row))


def test_data_gradient_refusals_launch_nothing():
    from accel_rl_amd import _lib
    lib = _lib.load()
    t = torch.zeros(4096, device=DEV)
    ok = _lib.conv_geom(2, 4, 4, 8, 32, 2, 2, 2, 0, 0)
    _lib.conv2d_bwd_data(t[:2 * 2 * 2 * 32], t[:32 * 2 * 2 * 8], None, t[2048:2048 + 2 * 4 * 4 * 8], ok)
    assert len(_log()) == 1                                              # (so that an empty log below is the refusal's)
    for bad, code, word in ((_lib.conv_geom(2, 7, 8, 8, 32, 3, 3, 2, 0, 0), -2, b"stride"),      # kernel 3, stride 2
                            (_lib.conv_geom(2, 7, 8, 6, 32, 2, 2, 2, 0, 0), -2, b"multiples of 4")):
        rc = lib.arl_conv2d_bwd_data(t.data_ptr(), t.data_ptr(), None, None, None, t.data_ptr(), _lib.C.byref(bad), None, None,
                                     None)
        assert rc == code and word in lib.arl_last_error() and _log() == []
        _lib.conv2d_bwd_data(t[:2 * 2 * 2 * 32], t[:32 * 2 * 2 * 8], None, t[2048:2048 + 2 * 4 * 4 * 8], ok)
        assert len(_log()) == 1


# ------------------------------------------------------------------------------------------------------------------
# weight gradient (+ bias gradient)
# ------------------------------------------------------------------------------------------------------------------
def _wg_kernels(K):
    """(split routes, FP32) launchers of a fast weight gradient by filter count."""
    if K <= 16:
        l = dict(family="wgrad_fast", tile=(1, 4, 1, 1, 32), flags="n16")
        return l, l
    if K <= 32:
        return dict(family="wgrad_split", tile=(1, 4, 1, 1, 32), minw=2), dict(family="wgrad_fast", tile=(1, 4, 1, 1, 32))
    if K <= 64:
        return dict(family="wgrad_split", tile=(2, 2, 1, 1, 32), minw=2), dict(family="wgrad_fast", tile=(2, 2, 1, 1, 32))
    return dict(family="wgrad_split", tile=(2, 2, 2, 2, 32), minw=1), dict(family="wgrad_fast", tile=(2, 2, 2, 2, 32))


def _wg_fast(row, splits, note=""):
    """A fast weight gradient: tiles of (16 | 32 | 64 | 128 filters) x (128 | 128 | 64 | 128 columns), `splits` row splits."""
    b, H, W, C, K, kh, kw, st, ph, pw = row
    bm, bn = (16, 128) if K <= 16 else (32, 128) if K <= 32 else (64, 64) if K <= 64 else (128, 128)
    grid = (-(-(kh * kw * C) // bn), -(-K // bm), splits)
    out = []
    for spec in _wg_kernels(K):
        spec = dict(spec)
        flags = spec.pop("flags", "") + (" has_pad" if ph or pw else "")
        out.append(launch(flags=flags, grid=grid, splits=splits, **spec))
    return dict(row=row, split=out[0], fp32=out[1], splits=splits, fast=True)


def _wg_generic(row, tile, grid, splits):
    l = launch("wgrad", tile, "", grid, splits)
    return dict(row=row, split=l, fp32=l, splits=splits, fast=False)


WGRAD = (
    # K_out = 4 .. 132 with C = 12 and 20: Mred = 288 (3 splits of 96 rows), 108 and 180 columns
    [_wg_fast((8, 6, 6, 12, K, 3, 3, 1, 1, 1), 3) for K in (4, 12, 16, 20, 36, 68, 132)] +
    [_wg_fast((8, 6, 6, 20, K, 3, 3, 1, 1, 1), 3) for K in (4, 20, 36, 132)] +
    [_wg_fast((7, 1, 32, 12, 20, 1, 3, 1, 0, 1), 2),                # Mred = 224: 2 splits of 128 and 96 rows
     _wg_fast((1, 1, 32, 4, 20, 1, 1, 1, 0, 0), 1),                 # Mred = 32: one k-tile, written in place
     _wg_fast((16384, 1, 1, 4, 4, 1, 1, 1, 0, 0), 128),             # 128 and 127 splits: either side of the wide fold
     _wg_fast((16256, 1, 1, 4, 4, 1, 1, 1, 0, 0), 127),
     # images of 1, 2, 255, 256, 257 and 300 output pixels around the 256 rows a workgroup advances by
     _wg_fast((64, 1, 1, 4, 20, 1, 1, 1, 0, 0), 1),
     _wg_fast((32, 1, 2, 4, 20, 1, 1, 1, 0, 0), 1),
     _wg_fast((32, 1, 255, 4, 20, 1, 3, 1, 0, 1), plan_split(1, 32 * 255, 512)[0]),
     _wg_fast((32, 1, 256, 4, 20, 1, 3, 1, 0, 1), plan_split(1, 32 * 256, 512)[0]),
     _wg_fast((32, 1, 257, 4, 20, 1, 3, 1, 0, 1), 65),
     _wg_fast((8, 1, 300, 4, 20, 1, 3, 1, 0, 1), plan_split(1, 8 * 300, 512)[0]),
     # Mred = 2 520 is no multiple of 32: generic kernels with splits, dbias not produced
     _wg_generic((9, 20, 14, 32, 20, 3, 3, 1, 1, 1), (1, 4, 1, 1, 16), (3, 1, 20), 20),
     # 49 taps with padding: generic
     _wg_generic((4, 8, 8, 32, 36, 7, 7, 1, 3, 3), (2, 2, 1, 1, 16), (25, 1, 2), 2)])


@pytest.mark.parametrize("case", WGRAD, ids=_ids(WGRAD))
def test_weight_gradient_at_every_dispatch_arm(case):
    from accel_rl_amd import _lib
    row = case["row"]
    b, H, W, C, K, kh, kw, st, ph, pw = row
    ho, wo = conv_ref.out_hw(row)
    x, w, _, dy, _ = _inputs(row, seed=2)
    refs = {False: conv_ref.wgrad(dy, x, row), True: conv_ref.wgrad(conv_ref.rounded(dy), conv_ref.rounded(x), row)}
    want_db = conv_ref.dbias(dy)
    ws = _lib.conv_workspace(DEV)
    errs = Errors(row)
    for route in ROUTES:
        geom = _geom(row, route)
        want_l = case["fp32" if route == "fp32" else "split"]
        outs = []
        for _ in range(2):
            dw, db = _nan(K, kh, kw, C), _nan(K)
            folds = _lib.FoldList()
            done = folds.conv2d_bwd_weight(dy, x, dw, geom, ws, dbias=db)
            got_log = _check_log([want_l], (row, route), SPLIT_MODE[route])
            folds.run()
            assert [g.family for g in _log()] == (["fold_many"] if case["splits"] > 1 or done else [])
            outs.append((dw, db))
        assert done == case["fast"], (row, route, "dbias is produced if and only if a fast kernel ran")
        assert torch.equal(outs[0][0], outs[1][0]), (row, route, "second run")
        rounded = route == "bf16" and got_log[0].family in PIECE_FAMILIES
        errs.check("wgrad", route, outs[0][0], refs[rounded], b * ho * wo)
        if done:
            assert torch.equal(outs[0][1], outs[1][1])
            errs.check("dbias", route, outs[0][1], want_db, b * ho * wo, rms=False)
        else:
            assert torch.isnan(outs[0][1]).all() and torch.isnan(outs[1][1]).all()
        # the entry point that folds by itself: the same kernel, its own fold launch (the wide one from 128 splits on)
        dw = _nan(K, kh, kw, C)
        _lib.conv2d_bwd_weight(dy, x, dw, geom, ws)
        _check_log([want_l] + ([fold(case["splits"], dw.numel())] if case["splits"] > 1 else []), (row, route, "folded"),
                   SPLIT_MODE[route])
        assert torch.equal(dw, outs[0][0]), (row, route, "arl_conv2d_bwd_weight against _parts + arl_fold_many")
    errs.split_routes_against_fp32()
    RAN.add(("wgrad", row))


# ------------------------------------------------------------------------------------------------------------------
# conv 1 from planar u8 observations
# ------------------------------------------------------------------------------------------------------------------
SCALE = float(np.float32(1.0 / 255.0))
U8_SPLIT = dict(family="igemm_split", tile=(4, 1, 2, 1, 32), flags="b_kc u8 direct", minw=2)      # 32-deep, 128-row tiles
U8_OCC = dict(family="igemm_occ", tile=(2, 2, 2, 1, 32), flags="b_kc u8 n16", minw=5)             # FP32: 64-row tiles
U8_N16 = dict(family="igemm_u8", tile=(4, 1, 2, 1, 16), flags="b_kc u8 n16")                      # <= 16 filters
U8_16DEEP = dict(family="igemm_u8", tile=(4, 1, 1, 1, 16), flags="b_kc u8")                       # 17 .. 32, 16-deep k-tiles


def _u8_case(rows, b, chw, K, kh, kw, st, fwd, wcfg, idx="random", offset=0, gather=None):
    """fwd: route -> launcher spec (its grid is ceil(M / rows-per-tile)); `img` = the image-stationary kernel;
    wcfg: route -> the weight-gradient plan (0 = 16-row tiles, 1 / 2 = split kernel on 256 / 128 columns, 3 = fp32 chain)."""
    return dict(rows=rows, b=b, chw=chw, K=K, kh=kh, kw=kw, st=st, fwd=fwd, wcfg=wcfg, idx=idx, offset=offset,
                gather=gather or U8_SPLIT,          # what runs in the image kernel's place under arl_dev_conv_variant(1)
                row=(rows, b, "x".join(map(str, chw)), K, kh, kw, st, idx, offset))


def _by_route(split, fp32, bf16=None):
    return dict(split9=split, split6=split, fp32=fp32, bf16=split if bf16 is None else bf16)


IMG = _by_route("img", U8_OCC, U8_SPLIT)
U8 = (
    # the image-stationary kernel (32 filters of 8 x 8) at 1, 256, 257, 513 and 769 images: one, two, three and four images
    # per workgroup (from three on the prefetch rotates both LDS buffers); rows through an index and in place
    [_u8_case(b + 3 if gathered else b, b if gathered else None, (1, 8, 16), 32, 8, 8, 4, IMG, _by_route(2, 3))
     for b in (1, 256, 257, 513, 769) for gathered in (True, False)] +
    [   # index rows 0 and rows - 1 repeated
        _u8_case(6, 40, (1, 8, 16), 32, 8, 8, 4, IMG, _by_route(2, 3), idx="ends"),
        # obs 4-byte but not 16-byte aligned: the image kernel declines
        _u8_case(5, None, (1, 8, 16), 32, 8, 8, 4, _by_route(U8_SPLIT, U8_OCC), _by_route(2, 3), offset=4),
        # filter counts (K = 16 of 8 x 8 also takes the image kernel, half its tile idle); 4 planes: 256 columns, plan 1
        _u8_case(5, None, (2, 8, 16), 4, 8, 8, 4, _by_route(U8_N16, U8_N16), _by_route(0, 0)),
        _u8_case(5, None, (2, 8, 16), 16, 8, 8, 4, _by_route("img", U8_N16, U8_N16), _by_route(0, 0), gather=U8_N16),
        _u8_case(5, None, (2, 8, 16), 20, 8, 8, 4, _by_route(U8_SPLIT, U8_OCC), _by_route(2, 3)),
        _u8_case(9, 7, (4, 8, 16), 32, 8, 8, 4, IMG, _by_route(1, 3)),
        # filter shapes: 4 x 4, 1 x 16 and 2 x 8 have no 32-deep k-tile of whole filter rows; 8 x 4 and 2 x 16 have
        _u8_case(5, None, (2, 8, 16), 20, 4, 4, 4, _by_route(U8_16DEEP, U8_16DEEP), _by_route(3, 3)),
        _u8_case(5, None, (2, 8, 16), 20, 1, 16, 4, _by_route(U8_16DEEP, U8_16DEEP), _by_route(2, 3)),
        _u8_case(5, None, (2, 8, 16), 20, 2, 8, 4, _by_route(U8_16DEEP, U8_16DEEP), _by_route(2, 3)),
        _u8_case(5, None, (2, 8, 16), 20, 8, 4, 4, _by_route(U8_SPLIT, U8_OCC), _by_route(3, 3)),
        _u8_case(5, None, (2, 8, 16), 20, 2, 16, 4, _by_route(U8_SPLIT, U8_OCC), _by_route(2, 3)),
    ])

U8_WGRAD = {0: dict(family="wgrad_u8", tile=(1, 4, 1, 1, 32), flags="u8 n16"),
            1: dict(family="wgrad_split", tile=(1, 4, 1, 2, 32), flags="u8", minw=2),
            2: dict(family="wgrad_split", tile=(1, 4, 1, 1, 32), flags="u8", minw=2),
            3: dict(family="wgrad_u8", tile=(1, 4, 1, 1, 32), flags="u8")}


def _u8_inputs(case):
    c, h, w = case["chw"]
    K, kh, kw = case["K"], case["kh"], case["kw"]
    rows, b = case["rows"], case["b"]
    gen = torch.Generator(device=DEV).manual_seed(rows)
    n = rows * c * h * w
    buf = torch.randint(0, 256, (n + 16,), device=DEV, generator=gen, dtype=torch.int32).to(torch.uint8)
    assert buf.data_ptr() % 16 == 0
    obs = buf[case["offset"]:case["offset"] + n].view(rows, c, h, w)
    idx = None
    if b is not None and case["idx"] == "ends":
        idx = torch.tensor([0, 0, rows - 1, rows - 1, 0, rows - 1, rows - 1, 0] * (b // 8), device=DEV, dtype=torch.int32)
    elif b is not None:
        idx = torch.randint(0, rows, (b,), device=DEV, generator=gen, dtype=torch.int32)
    wt = torch.randn(K, c, kh, kw, device=DEV, generator=gen) / np.sqrt(kh * kw * c)
    bias = torch.randn(K, device=DEV, generator=gen)
    row = (rows if b is None else b, h, w, c, K, kh, kw, case["st"], 0, 0)
    ho, wo = conv_ref.out_hw(row)
    dy = torch.randn(row[0], ho, wo, K, device=DEV, generator=gen)
    return obs, idx, wt, bias, dy, row


def _u8_fwd_launch(spec, row, variant, gather=None):
    ho, wo = conv_ref.out_hw(row)
    m = row[0] * ho * wo
    if spec == "img" and not variant:
        return launch("conv1_img", (0, 0, 0, 0, 0), "b_kc u8", (min(row[0], 256), 1, 1))
    if spec == "img":                                   # arl_dev_conv_variant(1): the tap-gathering kernel it replaces
        spec = gather
    per = spec["tile"][0] * spec["tile"][2] * (16 if "n16" in spec["flags"] else 32)
    return launch(grid=(-(-m // per), 1, 1), **spec)


@pytest.mark.parametrize("case", U8, ids=_ids(U8))
def test_u8_conv1_at_every_dispatch_arm(case):
    from accel_rl_amd import _lib
    lib = _lib.load()
    obs, idx, wt, bias, dy, row = _u8_inputs(case)
    b, H, W, C, K, kh, kw, st = row[:8]
    ho, wo = conv_ref.out_hw(row)
    ws = _lib.conv_workspace(DEV)
    fwd_refs = {r: conv_ref.fwd_u8(obs, idx, SCALE, conv_ref.rounded(wt) if r else wt, bias, row, True) for r in (False, True)}
    wg_refs = {r: conv_ref.wgrad_u8(conv_ref.rounded(dy) if r else dy, obs, idx, SCALE, row) for r in (False, True)}
    errs = Errors(case["row"])
    for route in ROUTES:
        geom = _geom(row, route)
        ys = []
        for variant in (0, 1):
            lib.arl_dev_conv_variant(variant)
            name = route + ("/gather kernels" if variant else "")
            for rep in range(2):
                y = _nan(b, ho, wo, K)
                _lib.conv2d_u8_fwd(obs, idx, SCALE, wt, bias, y, geom, True)
                got_log = _check_log([_u8_fwd_launch(case["fwd"][route], row, variant, case["gather"])], (case["row"], name), SPLIT_MODE[route])
                ys.append(y)
            # (the pixels are exact in one bf16 piece: on route BF16 only the weights are rounded)
            rounded = route == "bf16" and got_log[0].family in PIECE_FAMILIES
            errs.check("u8fwd", name, y, fwd_refs[rounded], kh * kw * C)
        lib.arl_dev_conv_variant(0)
        assert torch.equal(ys[0], ys[1]) and torch.equal(ys[2], ys[3]), (case["row"], route, "second run")
        # the tap-gathering split kernel issues the image kernel's piece products in its order: the same bits (16 filters of
        # 8 x 8 fall to the fp32 chain's 16-wide tiles instead: the float64 bound above)
        if case["fwd"][route] != "img" or case["gather"] is U8_SPLIT:
            assert torch.equal(ys[0], ys[2]), (case["row"], route, "gather kernels")
        # ---- weight gradient
        cfg = case["wcfg"][route]
        bm, bn = (16 if K <= 16 else 32), (256 if cfg == 1 else 128)
        splits = plan_split(-(-K // bm) * -(-(C * kh * kw) // bn), b * ho * wo, (4 if K <= 16 else 2) * 256)[0]
        want_l = launch(grid=(-(-(C * kh * kw) // bn), -(-K // bm), splits), splits=splits, **U8_WGRAD[cfg])
        outs = []
        for rep in range(2):
            dw, db = _nan(K, C, kh, kw), _nan(K)
            folds = _lib.FoldList()
            assert folds.conv2d_u8_bwd_weight(dy, obs, idx, SCALE, dw, geom, ws, dbias=db)
            got_log = _check_log([want_l], (case["row"], route, "wgrad"), SPLIT_MODE[route])
            folds.run()
            outs.append((dw, db))
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), (case["row"], route)
        rounded = route == "bf16" and got_log[0].family in PIECE_FAMILIES
        errs.check("u8wgrad", route, outs[0][0], wg_refs[rounded], b * ho * wo)
        errs.check("u8dbias", route, outs[0][1], conv_ref.dbias(dy), b * ho * wo, rms=False)
    errs.split_routes_against_fp32()
    RAN.add(("u8", case["row"]))


def test_u8_conv1_refuses_36_filters_and_launches_nothing():
    from accel_rl_amd import _lib
    lib = _lib.load()
    case = _u8_case(5, None, (2, 8, 16), 32, 8, 8, 4, None, None)
    obs, idx, wt, bias, dy, row = _u8_inputs(case)
    y = _nan(5, 1, 3, 36)
    _lib.conv2d_u8_fwd(obs, None, SCALE, wt, bias, y[..., :32].contiguous(), _geom(row, "split9"), True)
    assert len(_log()) == 1
    bad = _lib.conv_geom(5, 8, 16, 2, 36, 8, 8, 4, 0, 0)
    w36 = torch.zeros(36, 2, 8, 8, device=DEV)
    assert lib.arl_conv2d_u8_fwd(obs.data_ptr(), 5, None, SCALE, w36.data_ptr(), None, y.data_ptr(), None, _lib.C.byref(bad), 1,
                                 None) == -2
    assert b"<= 32 filters" in lib.arl_last_error() and _log() == []
    assert torch.isnan(y).all()
    item, bitem = _lib.ArlFoldItem(), _lib.ArlFoldItem()
    ws = _lib.conv_workspace(DEV)
    rc = lib.arl_conv2d_u8_bwd_weight_parts(y.data_ptr(), obs.data_ptr(), 5, None, SCALE, w36.data_ptr(), _lib.C.byref(bad),
                                            ws.data_ptr(), ws.numel() * 4, _lib.C.byref(item), None, None, None, None)
    assert rc == -2 and _log() == []


# ------------------------------------------------------------------------------------------------------------------
# census: every launcher instantiation of csrc/mfma_dispatch.h (ARL_P1 .. ARL_P7) is produced by a case above, or is
# listed as unreachable with the reason
# ------------------------------------------------------------------------------------------------------------------
def _inst(family, tile, key="", minw=0):
    """An entry of the lists, in _instantiation's form."""
    return (family, tuple(tile), frozenset(key.split()), minw)


INSTANTIATIONS = {
    "P1": [_inst("igemm_split", (4, 1, 2, 1, 32), "b_kc u8", 2), _inst("igemm_split", (4, 1, 1, 2, 32), "b_kc", 2),
           _inst("igemm_split", (4, 1, 1, 1, 32), "b_kc", 2)],
    "P2": [_inst("igemm_split", (2, 2, 2, 2, 32), "b_kc", 1), _inst("igemm_split", (2, 2, 1, 1, 32), "b_kc", 3),
           _inst("igemm_split", (2, 2, 1, 1, 32), "", 3)],
    "P3": [_inst("igemm_split", (4, 1, 1, 2, 32), "", 2), _inst("igemm_split", (4, 1, 1, 1, 32), "", 2),
           _inst("igemm_split", (2, 2, 2, 2, 32), "", 1)],
    "P4": [_inst("wgrad_split", (2, 2, 2, 2, 32), "", 1), _inst("wgrad_split", (2, 2, 1, 1, 32), "", 2),
           _inst("wgrad_split", (1, 4, 1, 1, 32), "", 2), _inst("wgrad_split", (1, 4, 1, 1, 32), "u8", 2),
           _inst("wgrad_split", (1, 4, 1, 2, 32), "u8", 2)],
    "P5": [_inst("bwd_pair", (2, 2, 2, 2, 32)), _inst("bwd_pair", (2, 2, 2, 2, 16))],
    "P6": [_inst("igemm", (2, 2, 1, 1, 32), "b_kc"), _inst("igemm", (2, 2, 1, 1, 32), ""),
           _inst("igemm", (2, 2, 2, 2, 32), "b_kc"), _inst("igemm", (2, 2, 2, 2, 32), ""),
           _inst("igemm", (4, 1, 2, 1, 16), "b_kc n16"), _inst("igemm", (4, 1, 2, 1, 16), "n16"),
           _inst("igemm", (4, 1, 1, 1, 32), "b_kc"), _inst("igemm", (4, 1, 1, 1, 16), "b_kc"),
           _inst("igemm", (4, 1, 1, 1, 16), "")],
    "P7": [_inst("igemm_occ", (2, 2, 2, 1, 32), "n16", 5), _inst("igemm_occ", (1, 4, 2, 1, 32), "b_kc n16", 5),
           _inst("igemm_occ", (1, 4, 2, 1, 32), "n16", 5), _inst("wgrad_fast", (2, 2, 2, 2, 32)),
           _inst("wgrad_fast", (2, 2, 1, 1, 32)), _inst("wgrad_fast", (1, 4, 1, 1, 32)),
           _inst("wgrad_fast", (1, 4, 1, 1, 32), "n16")],
}
UNREACHABLE = {
    _inst("igemm", (2, 2, 1, 1, 32), "b_kc"):
        "fwd_impl: N <= 64 with splits > 1 (splits are planned from N >= 128 on) or `small` on route FP32 (that is small32)",
    _inst("igemm", (4, 1, 1, 1, 32), "b_kc"):
        "fwd_impl: N <= 32 on route FP32 without the 16-deep condition, which every fast-path shape meets",
    _inst("igemm", (4, 1, 1, 1, 16), ""):
        "dgrad_impl: the second N <= 32 arm, behind N <= 16 and 16 < N <= 32",
}


def _expected_launches():
    for c in FWD + DGRAD:
        for key in ("split", "fp32", "generic", "wt", "pair_split", "pair_fp32"):
            for l in c.get(key) or ():
                yield l
    for c in WGRAD:
        yield c["split"]
        yield c["fp32"]
    for c in U8:
        for route in ROUTES:
            spec = c["fwd"][route]
            yield launch(**(c["gather"] if spec == "img" else spec))      # (img: its arl_dev_conv_variant(1) pass)
            yield launch(**U8_WGRAD[c["wcfg"][route]])


def test_census_of_the_launcher_instantiations():
    """The launches the cases ASSERT (every one of them is compared with the launch log when its case runs) cover
    ARL_P1 .. ARL_P7 but for the entries of UNREACHABLE; and when every case above has run in this session, so do the
    launches the logs actually showed, none of them an `unreachable` one."""
    produced = {_instantiation(l) for l in _expected_launches()}
    listed = [i for part in sorted(INSTANTIATIONS) for i in INSTANTIATIONS[part]]
    assert len(listed) == len(set(listed)) == 32
    missing = [i for i in listed if i not in produced and i not in UNREACHABLE]
    assert not missing, missing
    both = [i for i in listed if i in produced and i in UNREACHABLE]
    assert not both, both
    assert set(UNREACHABLE) <= set(listed) and len(UNREACHABLE) == 3
    all_cases = ({("fwd", c["row"]) for c in FWD} | {("dgrad", c["row"]) for c in DGRAD} | {("wgrad", c["row"]) for c in WGRAD} |
                 {("u8", c["row"]) for c in U8})
    print("cases run: %d of %d; unreachable: %s" % (len(RAN), len(all_cases), sorted(i[:2] + (sorted(i[2]),) for i in UNREACHABLE)))
    assert not set(UNREACHABLE) & SEEN
    if RAN == all_cases:
        assert not [i for i in listed if i not in SEEN and i not in UNREACHABLE]
