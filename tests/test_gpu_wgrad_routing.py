"""Which kernel the weight-gradient dispatch runs (csrc/conv_mfma.hip wgrad_plan and its consumer wgrad_launch): one case
per kernel family and per instantiation reachable under the default switches, at the smallest shape that reaches it.
Every case first asserts the launch log exactly - the names carry the instantiation - and then compares dW (and dW2 of
the pair form, db of the bias form) with a float64 CPU reference on operands rounded to the storage type, at the
weight-gradient tolerance of tests/test_gpu_pairs.py and tests/test_gpu_inner_boundaries.py (2e-3 of the gradient's
maximum + 1e-3: fp32 accumulation over up to a million positions).  The expected names were recorded from the dispatch as
it stood before the plan was folded into one function.  The staged and generic families are held by
tests/test_gpu_inner_boundaries.py and tests/test_gpu_parity.py.  Run with `-m gpu`."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no HIP device", allow_module_level=True)

import _native as N  # noqa: E402
import _ops as ops  # noqa: E402

DEV = torch.device("cuda:0")
F = torch.nn.functional
BF, F32 = torch.bfloat16, torch.float32
F16 = torch.float16
RTOL, ATOL = 2e-3, 1e-3
WIDE = 1024     # "wide": x is channels [0, cin) of a buffer this wide - a sample of 2^30 elements, past the LDS-DMA offsets


def _close(a, b, what):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = (a - b).abs().max().item()
    lim = ATOL + RTOL * max(b.abs().max().item(), 1e-30)
    print("%s: max err %.3e, limit %.3e" % (what, err, lim))
    assert err <= lim, "%s: max err %.3e > %.3e" % (what, err, lim)


def _wgrad_ref(gathered, dense, k, stride):
    """dW[o][i][tap] = sum_{n, p} dense[n, o, p] * gathered[n, i, stride * p + tap - k // 2] as k^3 float64 matrix
    products.  A Conv3d's weight gradient with (x, dy); a ConvTranspose3d(k3, s2, p1)'s with (dy, x), which gives
    [Cin][Cout][3][3][3] directly."""
    pad = k // 2
    gp = F.pad(gathered.double(), (pad,) * 6)
    n, co, do, ho, wo = dense.shape
    ci = gathered.shape[1]
    dm = dense.double().permute(1, 0, 2, 3, 4).reshape(co, -1)
    out = torch.empty(co, ci, k, k, k, dtype=torch.float64)
    for kd in range(k):
        for kh in range(k):
            for kw in range(k):
                sl = gp[:, :, kd:kd + stride * (do - 1) + 1:stride, kh:kh + stride * (ho - 1) + 1:stride,
                        kw:kw + stride * (wo - 1) + 1:stride]
                out[:, :, kd, kh, kw] = dm @ sl.permute(0, 2, 3, 4, 1).reshape(-1, ci)
    return out


# id: (what, dtype, n, cin, cout, x extents, k, stride, names).  what: "conv" (ru3d_conv3d_wgrad), "pair" (+ the 1x1x1
# conv's gradient from the same pass), "bias" (+ db), "convt" (ConvTranspose3d: x has the extents given, dy twice them),
# "split" (x as the two planes of a concat), "dw4" (dw 4 bytes off 16-byte alignment), "wide" (see WIDE)
R64, R8 = "wgrad_reduce<64>", "wgrad_reduce<8>"
CASES = {
    # the sliding kernel, 64 -> 64: a full last column, a light one (16 of 32 wide), a masked one that is not light
    "slide": ("conv", BF, 2, 64, 64, (32, 32, 64), 3, 1, ["wgrad3_s1_slide", R64]),
    "slide_pair": ("pair", BF, 2, 64, 64, (32, 32, 64), 3, 1, ["wgrad3_s1_slide<pair>", R64, R64]),
    "slide_light": ("conv", BF, 2, 64, 64, (32, 32, 48), 3, 1, ["wgrad3_s1_slide<edge>", R64]),
    "slide_light_pair": ("pair", BF, 2, 64, 64, (32, 32, 48), 3, 1, ["wgrad3_s1_slide<edge,pair>", R64, R64]),
    "slide_masked": ("conv", BF, 2, 64, 64, (32, 32, 56), 3, 1, ["wgrad3_s1_slide<edge>", R64]),
    "slide_masked_pair": ("pair", BF, 2, 64, 64, (32, 32, 56), 3, 1, ["wgrad3_s1_slide<edge,pair>", R64, R64]),
    "slide_two_pairs": ("conv", BF, 2, 32, 64, (32, 64, 64), 3, 1, ["wgrad3_s1_slide", R8]),
    "slide_split_x": ("split", BF, 2, 64, 32, (32, 64, 64), 3, 1, ["wgrad3_s1_slide", R8]),
    # the stride-1 tile kernel: slabs + reduce; a lone workgroup per pair stores dw itself unless dw is misaligned
    "tile_w8": ("conv", BF, 1, 64, 64, (8, 8, 8), 3, 1, ["wgrad3_s1_mfma<4,8,8>", R64]),
    "tile_w8_direct": ("conv", BF, 1, 512, 512, (8, 8, 8), 3, 1, ["wgrad3_s1_mfma<4,8,8>"]),
    "tile_w8_direct_dw4": ("dw4", BF, 1, 512, 512, (8, 8, 8), 3, 1, ["wgrad3_s1_mfma<4,8,8>", "wgrad_reduce_tiled<true>"]),
    "tile_w16": ("conv", BF, 1, 64, 64, (2, 8, 16), 3, 1, ["wgrad3_s1_mfma<2,8,16>"]),
    "tile_w32": ("conv", BF, 1, 64, 64, (2, 4, 32), 3, 1, ["wgrad3_s1_mfma<2,4,32>"]),
    # stride 2: the LDS-DMA kernel with two cout tiles per workgroup (Cout % 64 == 0) or one, the register-staged kernel
    # where a sample is past the DMA kernel's 2^30-element offsets, and ConvTranspose3d with its swapped operands
    "s2_dma2": ("conv", BF, 2, 64, 64, (32, 32, 32), 3, 2, ["wgrad3_s2_dma<2>", R8]),
    "s2_dma2_pair": ("pair", BF, 2, 64, 64, (32, 32, 32), 3, 2, ["wgrad3_s2_dma<2,pair>", R8, R8]),
    "s2_dma1": ("conv", BF, 2, 64, 96, (16, 16, 32), 3, 2, ["wgrad3_s2_dma<1>", R64]),
    "s2_dma1_pair": ("pair", BF, 2, 64, 96, (16, 16, 32), 3, 2, ["wgrad3_s2_dma<1,pair>", R64, R64]),
    "s2_tile": ("wide", BF, 1, 32, 32, (64, 128, 128), 3, 2, ["wgrad3_s2_tile", R8]),
    "convt_dma": ("convt", BF, 2, 64, 64, (16, 16, 16), 3, 2, ["wgrad3_s2_dma<2>", R8]),
    # stem (ragged H and W: masked border tiles) and head
    "stem_mfma": ("conv", BF, 2, 1, 32, (6, 12, 40), 3, 1, ["stem_wgrad_mfma", R64]),
    "stem_mfma_bias": ("bias", BF, 2, 1, 32, (6, 12, 40), 3, 1, ["stem_wgrad_mfma", R64, R64]),
    "stem_fp32": ("conv", F32, 2, 1, 32, (6, 12, 40), 3, 1, ["stem_wgrad", R64]),
    "head": ("conv", BF, 2, 32, 3, (8, 16, 32), 1, 1, ["head_wgrad", R64]),
}


@functools.lru_cache(maxsize=None)
def _operands(what, dt, n, cin, cout, dims, k, stride):
    """(x, dy, dy2) as fp32 values already rounded to the storage type, and the float64 references (dW, dW2, db):
    shared by the cases that differ only in the entry point, and never modified"""
    g = torch.Generator().manual_seed(n + cin + cout + sum(dims) + k + stride)
    ydims = tuple(2 * s for s in dims) if what == "convt" else tuple((s - 1) // stride + 1 for s in dims)
    xv = torch.randn((n, cin) + dims, generator=g).to(dt).float()
    g1 = torch.randn((n, cout) + ydims, generator=g).to(dt).float()
    g2 = torch.randn((n, cout) + ydims, generator=g).to(dt).float()
    if what == "convt":
        return xv, g1, g2, _wgrad_ref(g1, xv, 3, 2), None, None
    return xv, g1, g2, _wgrad_ref(xv, g1, k, stride), _wgrad_ref(xv, g2, 1, stride), g1.double().sum(dim=(0, 2, 3, 4))


# every 16-bit case in both storage types (same names: the fp16 build is a second compilation of the same dispatch); the
# fp32 stem case once
ROUTES = [(case, CASES[case][1]) for case in sorted(CASES)] + [(case, F16) for case in sorted(CASES) if CASES[case][1] == BF]


@pytest.mark.parametrize("case,dt", ROUTES, ids=[c + "-fp16" if t == F16 else c for c, t in ROUTES])
def test_wgrad_routing(case, dt):
    what, _, n, cin, cout, dims, k, stride, names = CASES[case]
    shared = what if what == "convt" else "conv"
    xv, g1, g2, ref, ref2, refb = _operands(shared, dt, n, cin, cout, dims, k, stride)
    if what == "split":        # [a | b] as two planes of one buffer
        x = N.Split(ops.as_input(torch.cat((xv[:, :cin // 2], xv[:, cin // 2:]), dim=0).to(DEV), dt))
    elif what == "wide":
        x = N.new_act(n, WIDE, dims[0], dims[1], dims[2], dt, DEV)[:, :cin]
        x.copy_(xv.to(DEV))
        assert dims[0] * dims[1] * dims[2] * WIDE >= 2 ** 30
    else:
        x = ops.as_input(xv.to(DEV), dt)
    dy = ops.as_input(g1.to(DEV), dt)
    dy2 = ops.as_input(g2.to(DEV), dt) if what == "pair" else None
    dw2 = db = None
    with ops.launch_log() as log:
        if what == "pair":
            both = ops.conv_wgrad_pair(x, dy, dy2, stride)
            assert both is not None, "no pair form for %s" % case
            dw, dw2 = both
        elif what == "bias":
            dw, db = ops.conv_wgrad_bias(x, dy, k, stride)
        elif what == "convt":
            dw = ops.convt_wgrad(x, dy)
        elif what == "dw4":
            buf = torch.empty(cout * cin * 27 + 1, dtype=torch.float32, device=DEV)
            ops.GRAD_ARENA[case] = buf[1:].view(cout, cin, 3, 3, 3)
            try:
                dw = ops.conv_wgrad(x, dy, k, stride, key=case)
            finally:
                del ops.GRAD_ARENA[case]
            assert dw.data_ptr() == buf.data_ptr() + 4 and dw.data_ptr() % 16 == 4
        else:
            dw = ops.conv_wgrad(x, dy, k, stride)
    print("ROUTE %s %s %s" % (case, dt, log.names))
    assert log.names == names
    _close(dw, ref, "%s dW" % case)
    if dw2 is not None:
        _close(dw2, ref2, "%s dW2" % case)
    if db is not None:
        _close(db, refb, "%s db" % case)
