"""Grouped bf16 weight gradients (kernels.wgrad_group, ensvs_conv_wgrad_bf16_group): G problems
of one shape in one launch against the same problems as single launches with the same split
count (bitwise), against float64, and inside the DiffNet backward (kernels.WGRAD_GROUP)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from ensemble_svs_with_interactions_amd import _lib as L
from ensemble_svs_with_interactions_amd import kernels as K

DEV = "cuda"
DILS = (1, 2, 4, 8, 16)
SHAPES = [(3, 517, 256, 512, 3),   # the 256 x 256 kernel: 18 of its tiles at G = 3
          (2, 333, 264, 296, 3),   # ragged N and K, 128 x 128 kernel
          (4, 250, 128, 128, 1),   # one tile per problem (bap residual half)
          (3, 200, 256, 256, 1),   # mgc residual half
          (1, 40, 256, 512, 3)]    # dil = 16: a split and a tap window cross the sequence ends


def rel(a, b):
    return ((a - b).abs().max() / (b.abs().max() + 1e-12)).item()


_OPS = {}


def operands(shape, G):
    """Seeded bf16 operands, made once per (shape, G) and never written: per problem its own
    x, and its dy as columns g*N .. of one wide buffer (ld = G*N, the DiffNet's d(pre)
    layout); per problem a dilation of its own for taps = 3."""
    if (shape, G) not in _OPS:
        B, T, Kc, N, taps = shape
        M = B * T
        gen = torch.Generator(device=DEV).manual_seed(1000 * G + N + Kc + T)
        assert Kc % 8 == 0 and N % 8 == 0  # bf16 rows of whole 16-B chunks
        Kp, ld = Kc, G * N
        xs = [K.cast_bf16(torch.randn(M, Kc, device=DEV, generator=gen), Kc, Kc, M)
              for _ in range(G)]
        dy = K.cast_bf16(torch.randn(M, ld, device=DEV, generator=gen), ld, ld, M)
        # 16, 1, 2, 4, 8: problem 0 takes the dilation longer than the shortest split
        dils = [DILS[(g + 4) % len(DILS)] if taps == 3 else 1 for g in range(G)]
        _OPS[(shape, G)] = (xs, Kp, dy, ld, dils)
    return _OPS[(shape, G)]


def run(shape, G, splits, grouped, accum, scale, fill):
    B, T, Kc, N, taps = shape
    xs, Kp, dy, ld, dils = operands(shape, G)
    dws = [torch.full((N, Kc, taps), fill, device=DEV) for _ in range(G)]
    sh = lambda g: -dils[g] * (taps // 2)  # noqa: E731
    if grouped:
        K.wgrad_group([dict(dy=dy, dyoff=g * N, x=xs[g], dst=dws[g], sn=Kc * taps, sk=taps, sj=1,
                            dil=dils[g], shift0=sh(g)) for g in range(G)],
                      ld, Kp, B, T, T, N, Kc, taps, L.PAD_ZERO, accum=accum, splits=splits,
                      scale=scale, defer=True)
    else:
        for g in range(G):
            K.wgrad(dy, ld, xs[g], Kp, B, T, T, N, Kc, taps, dils[g], sh(g), L.PAD_ZERO, dws[g],
                    Kc * taps, taps, 1, accum=accum, dtype=L.DT_BF16, dyoff=g * N, splits=splits,
                    scale=scale, defer=True)
    return dws


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("G", [3, 5])
@pytest.mark.parametrize("splits", [1, 2, 5])
def test_grouped_equals_single_launches_bitwise(shape, G, splits):
    """Every problem of a grouped launch has the bits of its own K.wgrad(..., splits=S):
    plain, accumulating with a scale into a pre-filled destination, and with the split
    reductions queued (K.deferred_wgrad).  One-tap shapes also against float64."""
    plain = [run(shape, G, splits, grouped, False, 1.0, 7.0) for grouped in (False, True)]
    acc = [run(shape, G, splits, grouped, True, 0.5, 0.25) for grouped in (False, True)]
    dfr = []
    for grouped in (False, True):
        with K.deferred_wgrad():
            dfr.append(run(shape, G, splits, grouped, True, 0.5, 0.25))
    torch.cuda.synchronize()
    for g in range(G):
        assert torch.equal(plain[0][g], plain[1][g]), g
        assert torch.equal(acc[0][g], acc[1][g]), g
        assert torch.equal(dfr[0][g], dfr[1][g]), g
        assert torch.equal(dfr[1][g], acc[1][g]), g
    B, T, Kc, N, taps = shape
    if taps == 1:
        xs, Kp, dy, ld, dils = operands(shape, G)
        for g in range(G):
            ref = torch.einsum("mn,mk->nk", dy[:, g * N:(g + 1) * N].double(),
                               xs[g][:, :Kc].double())
            assert rel(plain[1][g][:, :, 0].double(), ref) < 1e-5, g
            assert rel(acc[1][g][:, :, 0].double() - 0.25, 0.5 * ref) < 1e-5, g


def test_group_longer_than_one_launch():
    """More problems than one launch holds (32) are cut into several launches."""
    shape, G = (1, 96, 128, 128, 1), 35
    outs = [run(shape, G, 2, grouped, False, 1.0, 0.0) for grouped in (False, True)]
    torch.cuda.synchronize()
    for g in range(G):
        assert torch.equal(outs[0][g], outs[1][g]), g


def _diffnet_backward(on, fewer_splits=False):
    from ensemble_svs_with_interactions_amd import diffsinger, engine
    C, Ln, B, T, E, Mc = 128, 4, 2, 256, 64, 16
    torch.manual_seed(5)
    mod = diffsinger.DiffNet(in_dim=Mc, encoder_hidden_dim=E, residual_layers=Ln,
                             residual_channels=C).to(DEV)
    torch.nn.init.normal_(mod.output_projection.weight, std=C ** -0.5)
    xin = torch.randn(B * T, Mc, device=DEV)
    cond = torch.randn(B * T, E, device=DEV)
    t = torch.randint(0, 100, (B,), device=DEV)
    R = torch.randn(B * T, Mc, device=DEV)
    old = dict(K.WGRAD_GROUP)
    K.WGRAD_GROUP.update(on=on, fewer_splits=fewer_splits)
    engine.set_gemm_precision("bf16")
    try:
        out, st = mod._fwd(xin, Mc, t, cond, E, B, T)
        assert len(st["XB"]) == Ln  # the bf16-operand route
        dcond = mod._bwd(st, R)
        torch.cuda.synchronize()
    finally:
        engine.set_gemm_precision("fp32")
        K.WGRAD_GROUP.update(old)
    return dcond, {k: p.grad.clone() for k, p in mod.named_parameters()}


def test_diffnet_backward_group_on_vs_off():
    """A small DiffNet (C = 128, L = 4, B = 2, T = 256, bf16 route) with the per-block weight
    gradients grouped and as single launches.  No activation path changes, so the conditioner
    gradient is bitwise equal.  By default a group takes its problems' own split counts: every
    parameter gradient is bitwise equal too.  With fewer_splits the split count follows the
    group's tiles, so the per-block weight gradients may differ by the order of fp32 sums --
    bounded by the bf16 route's gradient tolerance of test_diffnet_gpu.py (rel-L2 < 1.5e-1);
    the measured figure is printed."""
    from golden_util import rel_l2
    dc_off, g_off = _diffnet_backward(False)
    dc_on, g_on = _diffnet_backward(True)
    assert torch.equal(dc_on, dc_off)
    for k in g_on:
        assert torch.equal(g_on[k], g_off[k]), k
    dc_few, g_few = _diffnet_backward(True, fewer_splits=True)
    assert torch.equal(dc_few, dc_off)
    errs = {k: rel_l2(g_few[k], g_off[k]) for k in g_few}
    print("fewer splits vs single weight gradients, largest rel-L2:",
          max(errs.items(), key=lambda kv: kv[1]))
    changed = [k for k in g_few if not torch.equal(g_few[k], g_off[k])]
    assert all("dilated_conv.weight" in k or "output_projection.weight" in k for k in changed), \
        changed
    for k, e in errs.items():
        assert e < 1.5e-1, (k, e)
