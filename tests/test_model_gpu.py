"""Module / block / model parity on a real MI355X against the golden vectors of the reference and the
CPU oracle.  fp32 mode must meet 1e-5 (relative to output max-abs); bf16 mode is compared with the same
fp32 goldens at the looser, per-test documented tolerance (the reference's OWN bf16 CPU forward deviates
from its fp32 forward by 1e-2 .. 1e-1 at the logits)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from detfill import det_tensor, fill_state_dict, sample
from oracle import lemevit_oracle as O
from test_oracle_golden import TRAIN_FIXTURES, block_spec, drop_path_plan

DEV = "cuda:0"


def L():
    import lemevit_amd
    return lemevit_amd


def close(out, ref, tol, what):
    out = np.asarray(out.detach().float().cpu().numpy() if torch.is_tensor(out) else out, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    assert out.shape == ref.shape, (what, out.shape, ref.shape)
    assert np.isfinite(out).all(), what
    mx = max(np.abs(ref).max(), 1e-30)
    err = np.abs(out - ref).max()
    assert err <= tol * mx, f"{what}: max-abs err {err:.3e} > {tol:.0e} * {mx:.3e}"
    return err / mx


def load(module, prefix, seed):
    spec = {prefix + k: tuple(v.shape) for k, v in module.state_dict().items()}
    sd = fill_state_dict(spec, seed)
    module.load_state_dict({k[len(prefix):]: v for k, v in sd.items()})
    return module.to(DEV)


MODES = [(torch.float32, 1e-5), (torch.bfloat16, 2e-2)]


@pytest.mark.parametrize("dtype,tol", MODES)
@pytest.mark.parametrize("name", ["dca_96", "dca_192", "dca_odd", "dca2_96"])
def test_dca_module(golden, name, dtype, tol):
    meta, g = golden(name)
    C, h, N, B = meta["C"], meta["h"], meta["N"], meta["B"]
    cls = L().DualCrossAttention_v2 if meta["kind"] == "dca2" else L().DualCrossAttention
    m = load(cls(dim=C, num_heads=h), "attn.", meta["seed"]).eval()
    pre = "dca2" if meta["kind"] == "dca2" else name
    x = det_tensor((B, N, C), pre + ".x", 1).to(DEV, dtype); c = det_tensor((B, 16, C), pre + ".c", 1).to(DEV, dtype)
    xo, co = m(x, c)
    close(sample(xo.float()), g["x_out"], tol, name + ".x"); close(co, g["c_out"], tol, name + ".c")


@pytest.mark.parametrize("dtype,tol", MODES)
@pytest.mark.parametrize("name", ["sa_384_196", "sa_384_16", "sa_odd"])
def test_sa_module(golden, name, dtype, tol):
    meta, g = golden(name)
    m = load(L().StandardAttention(dim=meta["C"], num_heads=meta["h"]), "attn.", meta["seed"]).eval()
    x = det_tensor((meta["B"], meta["L"], meta["C"]), name + ".x", 1).to(DEV, dtype)
    close(sample(m(x).float(), 16384), g["x_out"], tol, name)


@pytest.mark.parametrize("dtype,tol", MODES)
@pytest.mark.parametrize("name", ["ca_96", "ca_odd"])
def test_ca_module(golden, name, dtype, tol):
    meta, g = golden(name)
    m = load(L().CrossAttention(dim=meta["C"], num_heads=meta["h"]), "attn.", meta["seed"]).eval()
    x = det_tensor((meta["B"], meta["N"], meta["C"]), name + ".x", 1).to(DEV, dtype); c = det_tensor((meta["B"], 16, meta["C"]), name + ".c", 1).to(DEV, dtype)
    close(m(x, c), g["c_out"], tol, name)


def _block(t, C, h, dp=0.0, mlp_ratio=4):
    return L().LeMeBlock(dim=C, attn_drop=0.0, proj_drop=0.0, drop_path=dp, attn_type=t, num_heads=h, mlp_ratio=mlp_ratio)


@pytest.mark.parametrize("dtype,tol", MODES)
@pytest.mark.parametrize("name", ["block_C", "block_D", "block_S"])
def test_block_forward(golden, name, dtype, tol):
    meta, g = golden(name)
    t, C, h, H, W, B = meta["type"], meta["C"], meta["h"], meta["H"], meta["W"], meta["B"]
    m = load(_block(t, C, h), "blk.", meta["seed"]).eval()
    x = det_tensor((B, C, H, W), name + ".x", 2).to(DEV, dtype); c = det_tensor((B, 16, C), name + ".c", 2).to(DEV, dtype)
    with torch.no_grad():
        xo, co = m(x, c)                     # reference signature: NCHW in / out
    close(sample(xo.float().contiguous(), 16384), g["x_out"], tol, name + ".x"); close(co, g["c_out"], tol, name + ".c")
    # The fixture holds 16384 strided samples of the image-token map; a bug confined to one tile could sit between them.  The FULL
    # tensor is therefore compared with the CPU oracle (itself pinned to the reference by the same fixture, tests/test_oracle_golden.py).
    sd = {"blk." + k: v.detach().double().cpu() for k, v in m.state_dict().items()}
    xt, _, _ = O.to_tokens(x.detach().double().cpu())
    xr, cr = O.leme_block(sd, "blk.", t, xt, c.detach().double().cpu(), H, W, h)
    close(xo, O.to_nchw(xr, H, W).numpy(), tol, name + ".x (full tensor vs oracle)"); close(co, cr.numpy(), tol, name + ".c (full tensor vs oracle)")


@pytest.mark.parametrize("name", ["blockgrad_D", "blockgrad_S", "blockgrad_C", "blockgrad_D2"])
def test_block_backward_fp32(golden, name):
    meta, g = golden(name)
    t, C, h, H, W, B = meta["type"], meta["C"], meta["h"], meta["H"], meta["W"], meta["B"]
    m = load(_block(t, C, h), "blk.", meta["seed"]).eval()
    x = det_tensor((B, C, H, W), name + ".x", 3).to(DEV).requires_grad_(True); c = det_tensor((B, 16, C), name + ".c", 3).to(DEV).requires_grad_(True)
    gx = det_tensor((B, C, H, W), name + ".gx", 3).to(DEV); gc = det_tensor((B, 16, C), name + ".gc", 3).to(DEV)
    xo, co = m(x, c)
    ((xo * gx).sum() + (co * gc).sum()).backward()
    close(xo, g["x_out"], 1e-5, "x_out"); close(co, g["c_out"], 1e-5, "c_out")
    close(x.grad, g["dx"], 2e-5, "dx"); close(c.grad, g["dc"], 2e-5, "dc")
    for k, p in m.named_parameters():
        ref = g["grad." + k]
        if np.abs(ref).max() == 0:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0
        else:
            close(p.grad, ref, 3e-5, "grad " + k)


def _rel(out, ref):
    """max-abs error of a tensor against its reference, relative to the reference's max-abs"""
    out = out.detach().double().cpu() if torch.is_tensor(out) else torch.as_tensor(np.asarray(out, dtype=np.float64))
    ref = ref.detach().double().cpu() if torch.is_tensor(ref) else torch.as_tensor(np.asarray(ref, dtype=np.float64))
    assert out.shape == ref.shape, (out.shape, ref.shape)
    assert torch.isfinite(out).all()
    return float((out - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


def _oracle_block(sd, t, h, Hs, xb, cb, gx, gc, autocast=False):
    """The oracle's LeMeBlock forward + backward in float64 (autocast: the same torch code from fp32 operands under stock torch.autocast(bfloat16) -- the
    yardstick of what bf16 operands cost this block; it never runs the library).  -> outputs and gradients, keyed like the native side."""
    dt = torch.float32 if autocast else torch.float64
    sd = {k: v.detach().to(dt).requires_grad_(True) for k, v in sd.items()}
    xr = xb.to(dt).requires_grad_(True); cr = cb.to(dt).requires_grad_(True)
    with torch.autocast("cpu", torch.bfloat16, enabled=autocast):
        xt, _, _ = O.to_tokens(xr)
        xo, co = O.leme_block(sd, "blk.", t, xt, cr, Hs, Hs, h)
        xo = O.to_nchw(xo, Hs, Hs)
    ((xo.to(dt) * gx.to(dt)).sum() + (co.to(dt) * gc.to(dt)).sum()).backward()
    res = {"x_out": xo.detach().double(), "c_out": co.detach().double(), "dx": xr.grad.double(), "dc": cr.grad.double()}
    for k, v in sd.items():
        if v.grad is not None and float(v.grad.abs().max()) > 0:
            res["grad " + k[len("blk."):]] = v.grad.double()
    return res


# (attention type, C, heads, token grid side, mlp_ratio): the four first cases are the widths the bf16 block backward has always been held to; the others are the shapes only
# lemevit_small_v2 (MLP ratio 3: hidden 384 / 768 through the fused MLP kernels in three / six 128-wide chunks, hidden 192 / 1536 through the per-launch GEMMs), lemevit_small
# (C = 320), lemevit_tiny_v2 (D2 at C = 192) and vit_tiny (self-attention over 576 + 16 tokens at C = 96: the whole-row long-key kernels) reach
BLOCK_CASES_OLD = [("D", 96, 3, 14, 4), ("S", 192, 6, 7, 4), ("C", 64, 2, 14, 4), ("D2", 96, 3, 14, 4)]
BLOCK_CASES_NEW = [("D", 128, 4, 12, 3), ("D", 64, 2, 12, 3), ("S", 256, 8, 6, 3), ("S", 512, 16, 3, 3), ("S", 320, 10, 3, 4), ("D2", 192, 6, 6, 4), ("S", 96, 3, 24, 4)]


def _block_case(t, C, h, Hs, ratio, dtype):
    """One block, forward + backward on the GPU in `dtype`, and the float64 oracle on the operands the kernels read -> (native, oracle, inputs for a yardstick run)."""
    B = 3
    bf = dtype == torch.bfloat16
    m = load(_block(t, C, h, mlp_ratio=ratio), "blk.", 5).eval()
    sd = {"blk." + k: v.detach().to(torch.bfloat16).float().cpu() if bf and ("attn." in k or "mlp." in k) and k.endswith("weight") else v.detach().float().cpu()
          for k, v in m.state_dict().items()}
    rnd = (lambda v: v.to(torch.bfloat16)) if bf else (lambda v: v)
    xb = rnd(det_tensor((B, C, Hs, Hs), "x", 9)); cb = rnd(det_tensor((B, 16, C), "c", 9))
    gx = rnd(det_tensor((B, C, Hs, Hs), "gx", 9)); gc = rnd(det_tensor((B, 16, C), "gc", 9))
    x = xb.to(DEV).requires_grad_(True); c = cb.to(DEV).requires_grad_(True)
    with torch.autocast("cuda", torch.bfloat16, enabled=bf):
        xo, co = m(x, c)
    ((xo.float() * gx.to(DEV).float()).sum() + (co.float() * gc.to(DEV).float()).sum()).backward()
    got = {"x_out": xo, "c_out": co, "dx": x.grad, "dc": c.grad}
    for k, p in m.named_parameters():
        got["grad " + k] = p.grad
    return got, _oracle_block(sd, t, h, Hs, xb, cb, gx, gc), (sd, xb, cb, gx, gc)


def _block_bf16_vs_oracle(t, C, h, Hs, ratio=4, admit=False):
    """-> the tensors over the budget, [(what, native error, yardstick error)]: 2e-2 of max-abs for the outputs, 3e-2 for every gradient.  admit: a tensor over it still passes
    inside 1.5 x the error of the oracle block's own torch code under stock bf16 autocast (differently rounded arithmetic of the same block, tests/test_train_dispatch_gpu.py)."""
    got, ref, (sd, xb, cb, gx, gc) = _block_case(t, C, h, Hs, ratio, torch.bfloat16)
    tag, over, yard = f"{t} C={C} {Hs}x{Hs} ratio {ratio}", [], None
    for k, r in ref.items():
        tol = 2e-2 if k in ("x_out", "c_out") else 3e-2
        e = _rel(got[k], r)
        print(f"bf16 block {tag}: {k} {e:.2e}")
        if e > tol:
            if yard is None:
                yard = _oracle_block(sd, t, h, Hs, xb, cb, gx, gc, autocast=True)
            ey = _rel(yard[k], r)
            print(f"bf16 block {tag}: {k} over {tol:.0e}; autocast oracle block {ey:.2e}")
            if not admit or e > 1.5 * ey:
                over.append((f"{tag} {k}", e, ey))
    return over


def test_block_backward_bf16_vs_oracle():
    """bf16 kernels: gradients of a D, S, C and D2 block vs the fp64 oracle on the same bf16-rounded inputs and weights; 2e-2 of each output's and 3e-2 of each gradient's
    max-abs (bf16 activations inside the block).  After the four widths this has always run come the shapes only the other registered variants reach (BLOCK_CASES_NEW).
    A tensor of those new shapes over the budget is admitted only within 1.5 x the error of the oracle block under stock bf16 autocast (_block_bf16_vs_oracle); none needs that so far."""
    over = []
    for case in BLOCK_CASES_OLD:
        over += _block_bf16_vs_oracle(*case)
    for case in BLOCK_CASES_NEW:
        over += _block_bf16_vs_oracle(*case, admit=True)
    assert not over, over


@pytest.mark.parametrize("t,C,h,Hs,ratio", BLOCK_CASES_NEW)
def test_block_backward_fp32_vs_oracle(t, C, h, Hs, ratio):
    """The fp32 block backward at the shapes no blockgrad_* fixture has (widths 96 .. 512, MLP ratio 3, D2 at C = 192, 592 keys), against the float64 oracle on the same
    weights and inputs, at the bounds of test_block_backward_fp32: outputs 1e-5, dx / dc 2e-5, parameter gradients 3e-5 of each tensor's max-abs."""
    got, ref, _ = _block_case(t, C, h, Hs, ratio, torch.float32)
    bad = []
    for k, r in ref.items():
        tol = 1e-5 if k in ("x_out", "c_out") else 2e-5 if k in ("dx", "dc") else 3e-5
        e = _rel(got[k], r)
        print(f"fp32 block {t} C={C} {Hs}x{Hs} ratio {ratio}: {k} {e:.2e}")
        if e > tol:
            bad.append((k, e, tol))
    assert not bad, bad
    for k, v in got.items():          # a parameter the oracle gives no gradient has none here either
        assert k in ref or v is None or float(v.abs().max()) == 0.0, k


def _model(variant, num_classes, seed, **kw):
    m = L().create_model(variant, num_classes=num_classes, **kw)
    spec = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    m.load_state_dict(fill_state_dict(spec, seed))
    return m.to(DEV)


@pytest.mark.parametrize("name", ["model_tiny_224", "model_base_224", "model_small_224", "model_tiny_384", "model_small_v2_224", "model_tiny_v2_224",
                                  "model_vit_tiny_224", "model_base_384"])
def test_model_forward_fp32(golden, name):
    """BASELINE config 1 + fp32 parity: logits within 1e-5 (rel. max-abs) of the reference's CPU forward."""
    meta, g = golden(name)
    m = _model(meta["variant"], meta["num_classes"], meta["seed"]).eval()
    assert len(m.state_dict()) == meta["nkeys"] and sum(p.numel() for p in m.parameters()) == meta["nparams"]
    img = det_tensor((meta["B"], 3, meta["res"], meta["res"]), name + ".img", 4).to(DEV)
    with torch.no_grad():
        logits = m(img)
    e = close(logits, g["logits"], 1e-5, name + " logits")
    print(f"{name}: fp32 logits rel err {e:.2e}")


def test_eval_conv_bn_folding_fp32(golden):
    """Under no_grad the stem / stage-transition BatchNorms are folded into their convolutions (model.py::_run_downsample);
    with grad enabled the eval forward runs conv and BatchNorm separately.  Both must meet the golden logits, and the
    folded weights must follow an in-place update of the BatchNorm statistics."""
    name = "model_tiny_224"
    meta, g = golden(name)
    m = _model(meta["variant"], meta["num_classes"], meta["seed"]).eval()
    img = det_tensor((meta["B"], 3, meta["res"], meta["res"]), name + ".img", 4).to(DEV)
    with torch.no_grad():
        folded = m(img)
    unfolded = m(img)                      # grad enabled: nn.Sequential path
    close(folded, g["logits"], 1e-5, "folded")
    close(unfolded, g["logits"], 1e-5, "unfolded")
    with torch.no_grad():
        m.downsample_layers[0][1].running_mean.add_(0.25)
        moved = m(img)
    ref = m(img)
    assert float((moved - folded).abs().max()) > 1e-4, "folded weights were not refreshed after the statistics changed"
    close(moved, ref.detach().cpu().numpy(), 1e-5, "refreshed fold")


@pytest.mark.parametrize("name", ["model_tiny_224", "model_base_224", "model_base_384"])       # model_base_384 = BASELINE config 5
@pytest.mark.parametrize("mode", ["autocast", "pure"])
def test_model_forward_bf16(golden, name, mode):
    """End-to-end bf16 (both benchmark.py flavours: --amp autocast, and --precision bfloat16 whole-model cast).
    Tolerance 5e-2 of the logits' max-abs: the reference's own bf16 CPU forward is 1.2e-2 (Tiny) / 1.2e-1 (Base) away
    from its fp32 forward in absolute terms."""
    meta, g = golden(name)
    m = _model(meta["variant"], meta["num_classes"], meta["seed"]).eval()
    img = det_tensor((meta["B"], 3, meta["res"], meta["res"]), name + ".img", 4).to(DEV)
    with torch.no_grad():
        if mode == "autocast":
            with torch.autocast("cuda", torch.bfloat16):
                logits = m(img)
        else:
            logits = m.to(torch.bfloat16)(img.to(torch.bfloat16))
    e = close(logits, g["logits"], 5e-2, f"{name} {mode}")
    print(f"{name} [{mode}]: bf16 logits rel err {e:.2e}")


@pytest.mark.parametrize("parts", [2, 3])
def test_split_forward_concurrent_sub_batches(parts):
    """lemevit_amd.graph.split_forward (the forward_* / --mode infer schedule of bench.py): the batch as concurrent sub-batches on forked
    streams, eager and as branches of one hipGraph, is BIT-equal to the same sub-batches run one after the other (the branches share
    no scratch), and within the bf16 end-to-end budget of the whole-batch result (other row counts select other kernels)."""
    from lemevit_amd.graph import GraphedStep, split_forward
    m = _model("lemevit_tiny", 1000, 3).eval()
    B = 11
    img = det_tensor((B, 3, 224, 224), "split.img", 4).to(DEV)
    with torch.no_grad(), torch.autocast("cuda", torch.bfloat16):
        whole = m(img)
        seq = torch.cat([m(xi) for xi in img.chunk(parts)])
        par = split_forward(m, img, parts)
    torch.cuda.synchronize()
    assert par.shape == whole.shape and torch.equal(par, seq)
    close(par, whole.float().cpu(), 5e-2, "sub-batches vs whole batch")
    outs = []

    def step():
        with torch.no_grad(), torch.autocast("cuda", torch.bfloat16):
            split_forward(m, img, parts, outs)

    g = GraphedStep(step, warmup=2)
    for _ in range(3):
        g()
    torch.cuda.synchronize()
    assert len(outs) == parts and torch.equal(torch.cat(outs), seq)


@pytest.mark.parametrize("variant", ["lemevit_tiny", "lemevit_base"])
def test_split_forward_cold_caches(variant):
    """the lazily built operand caches (bf16 casts, LayerNorm folds, conv + BatchNorm folds, the classifier tail, the packed S
    stage) are filled by the FIRST sub-batch; the other sub-batch streams must not read them before those kernels have run.  A fresh model
    (every cache cold) goes straight into split_forward, again after new_training_pass() (what the first eval batch after a training pass
    sees), under a busy chip -- the result must be bit-equal to the warm sequential sub-batches."""
    import lemevit_amd.model as M
    from lemevit_amd.graph import split_forward
    m = _model(variant, 1000, 5).eval()
    B, parts = 12, 4
    img = det_tensor((B, 3, 224, 224), "split.cold", 4).to(DEV)
    busy = torch.randn(4096, 4096, device=DEV)
    with torch.no_grad(), torch.autocast("cuda", torch.bfloat16):
        for _ in range(4):
            busy = busy @ busy * 1e-3                 # keeps the main stream behind: the forked streams would run ahead of a cold cache fill
        cold = split_forward(m, img, parts)
        torch.cuda.synchronize()
        seq = torch.cat([m(xi) for xi in img.chunk(parts)])
        assert torch.equal(cold, seq), float((cold.float() - seq.float()).abs().max())
        M.new_training_pass()                          # stamps move: every cache is rebuilt by the next pass
        for _ in range(4):
            busy = busy @ busy * 1e-3
        cold2 = split_forward(m, img, parts)
        torch.cuda.synchronize()
        assert torch.equal(cold2, seq), float((cold2.float() - seq.float()).abs().max())


@pytest.mark.parametrize("name", ["model_tiny_224", "model_base_224", "model_small_v2_224", "model_tiny_v2_224"])
def test_fused_inference_path(golden, name, monkeypatch):
    """The inference schedule with LayerNorm folded into the projections and the one-kernel MLP half (lmv_ln_linear_fwd /
    lmv_mlp_fused_fwd through LMV_BLOCK_FUSED, and the Python schedule of the "D2" blocks) against the golden logits of the
    reference AND against the unfused schedule of the same model: both must sit inside the bf16 end-to-end budget, and the
    two schedules within 3e-2 of each other (they round at different places: gamma . W instead of W and LN(x))."""
    import lemevit_amd.model as M
    meta, g = golden(name)
    m = _model(meta["variant"], meta["num_classes"], meta["seed"]).eval()
    img = det_tensor((meta["B"], 3, meta["res"], meta["res"]), name + ".img", 4).to(DEV)
    outs = {}
    for fused in (True, False):
        monkeypatch.setattr(M, "_FUSED", fused)
        with torch.no_grad(), torch.autocast("cuda", torch.bfloat16):
            outs[fused] = m(img).float()
    e1 = close(outs[True], g["logits"], 5e-2, f"{name} fused")
    e0 = close(outs[False], g["logits"], 5e-2, f"{name} unfused")
    ref = outs[False].abs().max().item()
    d = (outs[True] - outs[False]).abs().max().item() / ref
    print(f"{name}: fused {e1:.2e} / unfused {e0:.2e} off the golden logits, fused vs unfused {d:.2e}")
    assert d <= 3e-2
    # the folded operands follow the parameters: perturb a LayerNorm affine and a fc1 weight in place (version bump) -> new logits
    blk = m.stages[3][0] if len(m.stages) > 3 else m.stages[-1][0]
    monkeypatch.setattr(M, "_FUSED", True)
    with torch.no_grad():
        blk.norm2.weight.mul_(1.5); blk.mlp[0].weight.add_(0.01)
        with torch.autocast("cuda", torch.bfloat16):
            a = m(img).float()
        monkeypatch.setattr(M, "_FUSED", False)
        with torch.autocast("cuda", torch.bfloat16):
            b = m(img).float()
    assert (a - outs[True]).abs().max().item() > 1e-3 * ref, "stale folded weights"
    assert (a - b).abs().max().item() <= 3e-2 * b.abs().max().item()




# ---- round 5: the attention modules as differentiable sub-boundaries (missing #5) -----------------------------------------
@pytest.mark.parametrize("dtype,tol", [(torch.float32, 2e-4), (torch.bfloat16, 3e-2)])
@pytest.mark.parametrize("kind", ["S", "D", "D2", "C"])
def test_attention_modules_are_differentiable(kind, dtype, tol):
    """StandardAttention / DualCrossAttention(_v2) / CrossAttention called on their own under autograd (models/lemevit.py:185,252,454 are ordinary nn.Modules): outputs and
    EVERY gradient -- inputs, weights, biases -- against the CPU oracle's autograd on the operands the kernels read.  (Rounds 1 - 4 decorated these forwards with no_grad: under
    autograd they silently returned constants.)"""
    lib = L()
    for C, h, B, N, M in ((96, 3, 2, 196, 16), (64, 2, 2, 49, 16)):          # C = 96 has a fused LayerNorm + projection launch (unused without norm1), C = 64 has none
        _check_attention_module(lib, kind, dtype, tol, C, h, B, N, M)


def _assert_nothing_deferred():
    """A stand-alone module launches its weight gradients in line: its backward leaves nothing on the side stream and no deferred join (the block schedules do both)."""
    from lemevit_amd import blocks
    assert not blocks._inflight and not any(blocks._pending.values()), (blocks._inflight, blocks._pending)


def _check_attention_module(lib, kind, dtype, tol, C, h, B, N, M):
    cls = {"S": lib.StandardAttention, "D": lib.DualCrossAttention, "D2": lib.DualCrossAttention_v2, "C": lib.CrossAttention}[kind]
    m = load(cls(dim=C, num_heads=h), "attn.", 77)
    if dtype == torch.bfloat16:          # the kernels read bf16 copies of the fp32 masters: give the oracle the same operands
        with torch.no_grad():
            for n_, p_ in m.named_parameters():
                if p_.dim() == 2:
                    p_.copy_(p_.to(torch.bfloat16).float())
    x0 = det_tensor((B, N, C), "attnmod.x", 5).to(dtype)
    c0 = det_tensor((B, M, C), "attnmod.c", 5).to(dtype)
    gx = det_tensor((B, N, C), "attnmod.gx", 6).to(dtype)
    gc = det_tensor((B, M, C), "attnmod.gc", 6).to(dtype)
    x = x0.to(DEV).requires_grad_(True)
    c = c0.to(DEV).requires_grad_(True)
    if kind == "S":
        out = m(x); loss = (out.float() * gx.to(DEV).float()).sum()
    elif kind == "C":
        out = m(x, c); loss = (out.float() * gc.to(DEV).float()).sum()
    else:
        ox, oc = m(x, c); loss = (ox.float() * gx.to(DEV).float()).sum() + (oc.float() * gc.to(DEV).float()).sum()
    loss.backward()
    _assert_nothing_deferred()
    # oracle (float64 autograd)
    sd = {"attn." + k: v.detach().double().cpu().requires_grad_(True) for k, v in m.state_dict().items()}
    xr = x0.double().requires_grad_(True); cr = c0.double().requires_grad_(True)
    if kind == "S":
        lr = (O.standard_attention(sd, "attn.", xr, h) * gx.double()).sum()
    elif kind == "C":
        lr = (O.cross_attention(sd, "attn.", xr, cr, h) * gc.double()).sum()
    else:
        fn = O.dual_cross_attention if kind == "D" else O.dual_cross_attention_v2
        a, b = fn(sd, "attn.", xr, cr, h)
        lr = (a * gx.double()).sum() + (b * gc.double()).sum()
    lr.backward()
    worst = close(x.grad, xr.grad.numpy(), tol, f"{kind} dx")
    if kind != "S":
        worst = max(worst, close(c.grad, cr.grad.numpy(), tol, f"{kind} dc"))
    for n_, p_ in m.named_parameters():
        assert p_.grad is not None, n_
        worst = max(worst, close(p_.grad, sd["attn." + n_].grad.numpy(), tol, f"{kind} {n_}"))
    print(f"attention module {kind} {dtype} C={C}: worst gradient error {worst:.2e}")
    if kind in ("D", "D2"):          # an unused output (its gradient arrives as None) must not break the node
        m.zero_grad()
        x2 = x0.to(DEV).requires_grad_(True)
        ox2, _ = m(x2, c0.to(DEV))
        (ox2.float() * gx.to(DEV).float()).sum().backward()
        _assert_nothing_deferred()
        assert torch.isfinite(x2.grad).all() and x2.grad.abs().max().item() > 0
    # and without autograd the module still takes the inference launches
    with torch.no_grad():
        o2 = m(x0.to(DEV)) if kind == "S" else m(x0.to(DEV), c0.to(DEV))
    o1 = out if kind in ("S", "C") else ox
    o2 = o2 if kind in ("S", "C") else o2[0]
    assert (o1.detach().float() - o2.float()).abs().max().item() <= 2e-2 * o2.float().abs().max().item()


def test_one_model_two_resolutions_packs_per_stage(monkeypatch):
    """stage 3 of one model instance resolves to the "S" kernel (sstage layout) at 14 x 14 tokens and to the "S2" kind of the D-stage kernel (dstage layout)
    at 24 x 24; that stage instance holds one derived pack per kind (model.derived, tag ("stage", kind)) and the ops refuse a foreign pack.  224 -> 384 -> 224 on one instance,
    each against the per-block schedule."""
    import lemevit_amd.model as M
    m = _model("lemevit_tiny", 10, 5).eval()
    imgs = {r: det_tensor((2, 3, r, r), f"tworez.{r}", 2).to(DEV) for r in (224, 384)}
    ref = {}
    monkeypatch.setattr(M, "_SSTAGE", False)
    with torch.no_grad(), torch.autocast("cuda", torch.bfloat16):
        for r, im in imgs.items():
            ref[r] = m(im).float()
    monkeypatch.setattr(M, "_SSTAGE", True)
    with torch.no_grad(), torch.autocast("cuda", torch.bfloat16):
        for r in (224, 384, 224, 384):
            out = m(imgs[r]).float()
            torch.cuda.synchronize()
            d = (out - ref[r]).abs().max().item() / ref[r].abs().max().item()
            assert d <= 3e-2, (r, d)
    kinds = sorted(tag[1] for owner, tag in M._derived if owner == id(m.stages[3]) and tag[0] == "stage")
    assert "S" in kinds and "S2" in kinds, kinds


def test_lost_handoff_is_loud(monkeypatch):
    """a persistent stage kernel whose bounded wait ran out sets the sticky error word; the NEXT forward call must raise (it reads the pinned
    word without a synchronisation), the word is cleared, and the process keeps to the per-block schedule from then on -- a wrong tensor never reaches the caller silently."""
    import lemevit_amd.model as M
    from lemevit_amd import _lib, ops
    m = _model("lemevit_tiny", 10, 5).eval()
    img = det_tensor((2, 3, 224, 224), "loud.img", 2).to(DEV)
    with torch.no_grad(), torch.autocast("cuda", torch.bfloat16):
        good = m(img).float()
    torch.cuda.synchronize()
    assert ops.stage_error_count() == 0
    monkeypatch.setattr(ops, "stage_kernels_disabled", False)
    _lib.check(_lib.lib.lmv_debug_stage_error_set(1), "lmv_debug_stage_error_set")          # what an exhausted in-launch wait does
    try:
        with pytest.raises(RuntimeError, match="hand-off"):
            with torch.no_grad(), torch.autocast("cuda", torch.bfloat16):
                m(img)
        assert ops.stage_kernels_disabled and ops.stage_error_count() == 0          # cleared; stage kernels off
        with torch.no_grad(), torch.autocast("cuda", torch.bfloat16):
            again = m(img).float()          # the per-block schedule
        torch.cuda.synchronize()
        assert (again - good).abs().max().item() <= 3e-2 * good.abs().max().item()
        # bench.py / graph.try_graphed call the same check at their synchronisation points
        _lib.check(_lib.lib.lmv_debug_stage_error_set(1), "lmv_debug_stage_error_set")
        with pytest.raises(RuntimeError):
            ops.check_stage_errors("test")
    finally:
        _lib.lib.lmv_debug_stage_error_set(0)
        ops.stage_kernels_disabled = False


def test_model_ema_matches_reference_rule():
    """Row f3 (optional EMA, main.py:316 / engine.py model_ema.update): after two optimizer steps every state_dict entry of ModelEma.module equals
    decay * ema + (1 - decay) * model applied twice (timm.utils.ModelEmaV2's rule), the block parameters through the one-launch flat kernel; and the EMA module runs the
    inference forward with ITS weights (no stale operand copies)."""
    lib = L()
    torch.manual_seed(0)
    m = _model("lemevit_tiny", 10, 11).train()
    opt = lib.FlatAdamW(m, lr=1e-2, weight_decay=0.05)
    decay = 0.9
    ema = lib.ModelEma(m, decay=decay, opt=opt)
    ref = {k: v.detach().clone().double() for k, v in m.state_dict().items() if v.dtype.is_floating_point}
    img = det_tensor((4, 3, 96, 96), "ema.img", 2).to(DEV)
    tgt = torch.tensor([1, 2, 3, 4], device=DEV)
    for _ in range(2):
        opt.zero_grad()
        with torch.autocast("cuda", torch.bfloat16):
            torch.nn.functional.cross_entropy(m(img), tgt).backward()
        opt.step()
        ema.update(m)
        for k, v in m.state_dict().items():
            if v.dtype.is_floating_point:
                ref[k] = decay * ref[k] + (1 - decay) * v.detach().double()
    torch.cuda.synchronize()
    got = ema.module.state_dict()
    for k, r in ref.items():
        close(got[k], r.cpu().numpy(), 1e-6, "ema " + k)
    assert int(got["norm.num_batches_tracked"]) == int(m.state_dict()["norm.num_batches_tracked"])
    m.eval()
    with torch.no_grad(), torch.autocast("cuda", torch.bfloat16):
        a, b = ema.module(img).float(), m(img).float()
    assert torch.isfinite(a).all() and (a - b).abs().max().item() > 0.0          # different weights -> different logits
    sd = {k: v.detach().cpu().float() if v.dtype.is_floating_point else v.detach().cpu() for k, v in got.items()}
    ref_logits = O.lemevit_forward(sd, O.VARIANTS["lemevit_tiny"], img.cpu())
    close(a, ref_logits.numpy(), 5e-2, "ema module forward")


def test_model_ema_update_with_wrapped_model():
    """The reference builds the EMA from the bare model and then calls model_ema.update(DistributedDataParallel(model)) (main.py:316, engine.py): the wrapper's state_dict keys
    carry a 'module.' prefix (update() raised KeyError there).  A wrapper with the same shape as DDP's -- an nn.Module holding the model as `.module` -- must give
    the same EMA as the bare model, and the source tensors are looked up once (not a state_dict() per step)."""
    lib = L()
    torch.manual_seed(0)
    m = _model("lemevit_tiny", 10, 11).train()
    opt = lib.FlatAdamW(m, lr=1e-2, weight_decay=0.05)
    ema_a, ema_b = lib.ModelEma(m, decay=0.9, opt=opt), lib.ModelEma(m, decay=0.9, opt=opt)

    class Wrapper(torch.nn.Module):          # DistributedDataParallel's layout without a process group
        def __init__(self, module):
            super().__init__()
            self.module = module

        def forward(self, *a, **k):
            return self.module(*a, **k)

    w = Wrapper(m)
    assert next(iter(w.state_dict())).startswith("module.")
    img = det_tensor((4, 3, 96, 96), "ema.img", 2).to(DEV)
    tgt = torch.tensor([1, 2, 3, 4], device=DEV)
    calls = []
    orig = type(m).state_dict
    for it in range(3):
        opt.zero_grad()
        with torch.autocast("cuda", torch.bfloat16):
            torch.nn.functional.cross_entropy(w(img), tgt).backward()
        opt.step()
        ema_a.update(m)
        if it == 1:          # from the second update on, no state_dict() of the source is built any more
            type(m).state_dict = lambda self, *a, **k: (calls.append(1), orig(self, *a, **k))[1]
        try:
            ema_b.update(w)
        finally:
            type(m).state_dict = orig
    torch.cuda.synchronize()
    assert not calls
    for (k, a), (_, b) in zip(ema_a.module.state_dict().items(), ema_b.module.state_dict().items()):
        assert torch.equal(a, b), k


def test_package_import_before_torch():
    """`import lemevit_amd` as the FIRST import of a fresh interpreter: the library must bind to the HIP runtime PyTorch-ROCm ships (round 5: loaded before torch it pulled
    /opt/rocm's copy and every launch failed with "no ROCm-capable device is detected"; lemevit_amd/_lib.py imports torch first now)."""
    import os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import lemevit_amd, torch\n"
            "m = lemevit_amd.create_model('lemevit_tiny', num_classes=10).cuda().eval()\n"
            "with torch.no_grad(), torch.autocast('cuda', torch.bfloat16):\n"
            "    y = m(torch.randn(2, 3, 224, 224, device='cuda'))\n"
            "torch.cuda.synchronize(); assert torch.isfinite(y.float()).all(); print('ok', tuple(y.shape))\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=root, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ok (2, 10)" in r.stdout, r.stderr[-2000:]


def test_launch_context_is_thread_local():
    """split_forward's sub-batch count used to be a module global that two inference threads raced on."""
    import threading
    import lemevit_amd.model as M
    seen = {}
    M.launches.concurrent = 4
    t = threading.Thread(target=lambda: seen.setdefault("other", M.launches.concurrent))
    t.start(); t.join()
    try:
        assert seen["other"] == 1 and M.launches.concurrent == 4
    finally:
        M.launches.concurrent = 1


@pytest.mark.parametrize("name", TRAIN_FIXTURES)
def test_train_step_fp32(golden, name):
    """Train-mode step of every registered variant but Base (BatchNorm batch statistics, DropPath with the reference's recorded masks): loss, logits, every
    parameter's gradient norm, selected full gradients and the updated BN running statistics against the reference's fixture; and -- a norm cannot see a permuted or
    sign-flipped gradient -- EVERY parameter's full gradient against the float64 oracle's autograd on the same weights, image and masks (the oracle is pinned to the
    same fixtures by tests/test_oracle_golden.py::test_train_step)."""
    meta, g = golden(name)
    cfg = O.VARIANTS[meta["variant"]]
    m = _model(meta["variant"], meta["num_classes"], meta["seed"], drop_path_rate=meta["drop_path_rate"]).train()
    plan = drop_path_plan(cfg, torch.from_numpy(g["dp_masks"])) if "dp_masks" in g else None
    if plan:
        assert len(m.stages) == len(cfg["depth"]) and [len(st) for st in m.stages] == list(cfg["depth"])
        for (i, j), rows in plan.items():          # two masks for a "C" block, four for "D" / "D2" / "S"
            assert m.stages[i][j].kind == cfg["attn_type"][i] and m.stages[i][j].drop_prob > 0.0
            fixed = [r.to(DEV).contiguous() for r in rows] + [None] * (4 - len(rows))
            m.stages[i][j]._masks = (lambda f: (lambda B, dev: f))(fixed)
        assert m.stages[0][0].drop_prob == 0.0 and (0, 0) not in plan
    img = det_tensor((meta["B"], 3, meta["res"], meta["res"]), name + ".img", 5).to(DEV)
    logits = m(img)
    loss = torch.nn.functional.cross_entropy(logits, torch.tensor(meta["target"], device=DEV))
    loss.backward()
    close(logits, g["logits"], 2e-5, "logits")
    assert abs(loss.item() - float(g["loss"])) < 2e-5
    params = dict(m.named_parameters())
    gn = np.array([float(params[k].grad.norm()) if params[k].grad is not None else 0.0 for k in meta["param_names"]])
    bad = np.abs(gn - g["grad_norms"]) > 1e-3 * np.maximum(1.0, np.abs(g["grad_norms"]))
    assert not bad.any(), [(meta["param_names"][i], gn[i], g["grad_norms"][i]) for i in np.nonzero(bad)[0][:5]]
    for k in g:
        if k.startswith("grad.") and k != "grad_norms":
            close(params[k[5:]].grad, g[k], 2e-4, k)
        if k.startswith("stat."):
            close(m.state_dict()[k[5:]], g[k], 1e-5, k)
    # every full gradient against the float64 oracle: 2e-4 of each tensor's max-abs (the bound of the listed gradients above); only tensors whose oracle gradient is
    # <= 1e-5 of the largest gradient max-abs are left out (mathematically zero: a conv bias in front of a train-mode BatchNorm, a k bias inside a softmax)
    sd = {k: v.double() for k, v in fill_state_dict(O.state_dict_spec(cfg, meta["num_classes"]), meta["seed"]).items()}
    for k, v in sd.items():
        if not k.endswith(("running_mean", "running_var", "num_batches_tracked")):
            v.requires_grad_(True)
    dplan = {key: [r.double() for r in rows] for key, rows in plan.items()} if plan else None
    ref_logits = O.lemevit_forward(sd, cfg, img.cpu().double(), train=True, dp_masks=dplan)
    torch.nn.functional.cross_entropy(ref_logits, torch.tensor(meta["target"])).backward()
    gmax = max(float(sd[k].grad.abs().max()) for k in params if sd[k].grad is not None)
    n, worst, over = 0, ("", 0.0), []
    for k, p in params.items():
        r = sd[k].grad
        if r is None or float(r.abs().max()) <= 1e-5 * gmax:
            continue
        assert p.grad is not None, k
        e = float((p.grad.detach().double().cpu() - r).abs().max() / r.abs().max())
        n += 1
        if e > worst[1]:
            worst = (k, e)
        if not e <= 2e-4:
            over.append((k, e))
    print(f"{name}: {n} of {len(params)} gradients vs the float64 oracle, worst {worst[1]:.2e} ({worst[0]})")
    assert not over, over[:8]
    assert n >= 0.95 * len(params), (n, len(params))


def _grad_stats(grads, ref, loss, ref_loss):
    """The statistics the bf16 end-to-end gradient tests assert on: `grads` {name: gradient} against the oracle gradients `ref` (the same keys; None = no gradient).  Tensors
    whose oracle gradient is <= 1e-5 of the largest gradient max-abs are left out of the per-tensor figures (mathematically zero gradients -- a conv bias in front of a
    train-mode BatchNorm, a k bias inside a softmax: rounding noise on both sides)."""
    worst_cos, errs = ("", 1.0), []
    gmax = max(float(r.abs().max()) for r in ref.values() if r is not None)
    for k, gq in grads.items():
        r = ref[k]
        if r is None or float(r.abs().max()) <= 1e-5 * gmax:
            continue
        gq = gq.detach().float().cpu()
        assert torch.isfinite(gq).all(), k
        e = float((gq - r).abs().max() / r.abs().max())
        c = float(torch.nn.functional.cosine_similarity(gq.flatten().double(), r.flatten().double(), dim=0))
        errs.append((e, float((gq - r).norm() / r.norm()), c, k))
        if c < worst_cos[1]:
            worst_cos = (k, c)
    errs.sort(reverse=True)
    gall = torch.cat([gq.detach().float().cpu().flatten() for k, gq in grads.items() if ref[k] is not None]).double()
    rall = torch.cat([ref[k].flatten() for k in grads if ref[k] is not None]).double()
    return dict(n=len(errs), errs=errs, loss=abs(loss - ref_loss) / abs(ref_loss), gl2=float((gall - rall).norm() / rall.norm()),
                gcos=float(torch.nn.functional.cosine_similarity(gall, rall, dim=0)), med=sorted(x[0] for x in errs)[len(errs) // 2],
                p90=sorted(x[0] for x in errs)[len(errs) * 9 // 10], worst_cos=worst_cos[1], worst_cos_name=worst_cos[0])


def _oracle_train_grads(cfg, sd, img, tgt, dtype, autocast=False):
    """loss and {name: gradient or None} of the oracle's train-mode step on the state dict `sd` (the module's forward has already moved the BatchNorm running statistics
    in it: the oracle's train-mode forward uses batch statistics, so that does not matter).  autocast: the same torch code under stock torch.autocast(bfloat16)."""
    ref_sd = {k: (v.detach().to(dtype).clone().requires_grad_(True) if v.dtype.is_floating_point and "running" not in k else v) for k, v in sd.items()}
    with torch.autocast("cpu", torch.bfloat16, enabled=autocast):
        logits = O.lemevit_forward(ref_sd, cfg, img.to(dtype), train=True)
    loss = torch.nn.functional.cross_entropy(logits.to(dtype), tgt)
    loss.backward()
    return loss.item(), {k: v.grad for k, v in ref_sd.items() if v.dtype.is_floating_point and "running" not in k}


def _bf16_train_grads(variant, num_classes, img, tgt):
    """One bf16-autocast train-mode step of the native model from the reference's own initialisation (models/lemevit.py:789-796: trunc_normal(0.02) Linears, LayerNorm (1, 0))
    -- what bench.py trains.  (The goldens' hash-filled weights are non-degenerate on purpose -- the residual stream reaches 6e4 there -- which is the right stress for forward
    parity and the wrong operating point for a bf16 gradient budget: with them 31 of 545 Base tensors exceed 5e-2, all column sums over the stage-3 residual-stream gradient.)
    -> loss, {name: gradient}, the CPU state dict."""
    torch.manual_seed(0)
    m = L().create_model(variant, num_classes=num_classes, drop_path_rate=0.0).to(DEV).train()
    with torch.autocast("cuda", torch.bfloat16):
        loss = torch.nn.functional.cross_entropy(m(img.to(DEV)), tgt.to(DEV))
    loss.backward()
    return loss.item(), {k: p.grad for k, p in m.named_parameters()}, {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}


# the project's accepted end-to-end bf16 budget (test_base_224_bf16_gradients_vs_oracle): loss, whole-gradient rel-L2 and cosine, per-tensor median and 90th percentile, worst cosine
BF16_BUDGET = dict(loss=3e-2, gl2=3e-2, gcos=0.9995, med=2e-2, p90=8e-2, worst_cos=0.90)


def test_base_224_bf16_gradients_vs_oracle():
    """the bf16 gradients of the headline configuration (LeMeViT-Base, 224 x 224, bf16 autocast, train mode, every stage at its real shape -- the
    full-size tests only checked them for finiteness) against the pinned oracle's fp32 autograd on the same weights and images, B = 4.  Per parameter tensor the error is taken
    relative to that tensor's gradient max-abs; the bound is the end-to-end bf16 budget (30 blocks of bf16 operands in both passes: measured ~1e-2 on the large tensors, a few
    1e-2 on the 16-token meta path), and the cosine against the oracle's gradient must be ~1 for every tensor that carries a gradient."""
    cfg = O.VARIANTS["lemevit_base"]
    img = det_tensor((4, 3, 224, 224), "basegrad.img", 5)
    tgt = torch.tensor([3, 141, 592, 653])
    loss, grads, sd = _bf16_train_grads("lemevit_base", 1000, img, tgt)
    ref_loss, ref = _oracle_train_grads(cfg, sd, img, tgt, torch.float32)
    assert abs(loss - ref_loss) <= 3e-2 * abs(ref_loss), (loss, ref_loss)
    st = _grad_stats(grads, ref, loss, ref_loss)
    print("largest per-tensor errors (max-abs, rel-L2, cosine):", [(k, round(e, 3), round(l2, 3), round(c, 4)) for e, l2, c, k in st["errs"][:8]])
    print(f"Base 224 bf16 gradients vs oracle, {st['n']} tensors: whole-gradient rel-L2 {st['gl2']:.2e}, cosine {st['gcos']:.5f}; per tensor median {st['med']:.2e}, "
          f"90th percentile {st['p90']:.2e}, worst cosine {st['worst_cos']:.4f} ({st['worst_cos_name']})")
    assert st["n"] >= 520
    # The step the optimizer takes: the whole gradient.  Per tensor the budget holds for the bulk; the tail is made of COLUMN SUMS OVER TOKENS of the residual-stream gradient
    # (pos_embed.bias = sum_t dx; proj_x.weight ~ (sum_t g) v-bar while the attention is still uniform at initialisation; the BatchNorm affine behind a stage): the train-mode
    # BatchNorm at the top makes that gradient sum to ~0 over tokens, so these entries are differences of cancelling terms and carry the bf16 rounding noise of ~N tokens against a
    # small true value -- in the reference's own autocast as well.  They are held to a direction test (cosine), not to the element budget.
    assert st["gl2"] <= 3e-2 and st["gcos"] >= 0.9995, (st["gl2"], st["gcos"])
    assert st["med"] <= 2e-2 and st["p90"] <= 8e-2, (st["med"], st["p90"])
    assert st["worst_cos"] >= 0.90, (st["worst_cos_name"], st["worst_cos"])


@pytest.mark.parametrize("variant", ["lemevit_tiny", "lemevit_small", "lemevit_small_v2", "lemevit_tiny_v2", "vit_tiny"])
def test_variant_96_bf16_gradients_vs_oracle(variant):
    """The bf16 train step of every other registered variant (96 x 96, B = 4, the reference's own initialisation, no DropPath, bf16 autocast) against the float64 oracle's
    autograd on the same weights and images: the statistics of the Base test.  Nobody had measured them at 9 .. 576 tokens, so each statistic passes inside the Base
    test's bound (BF16_BUDGET) OR inside 1.5 x the same statistic of a yardstick -- the oracle's own torch code under stock torch.autocast(bfloat16) on the CPU, against the
    same float64 gradients (cosines: 1.5 x its deficit from 1).  1.5 is the margin tests/test_train_dispatch_gpu.py grants a differently rounded form of the same arithmetic;
    the yardstick never runs the library.  One run is recorded in profiles/train_variants_parity.txt."""
    cfg = O.VARIANTS[variant]
    img = det_tensor((4, 3, 96, 96), "variantgrad.img", 5)
    tgt = torch.tensor([1, 7, 3, 3])
    loss, grads, sd = _bf16_train_grads(variant, 10, img, tgt)
    ref_loss, ref = _oracle_train_grads(cfg, sd, img, tgt, torch.float64)
    yloss, ygrads = _oracle_train_grads(cfg, sd, img, tgt, torch.float32, autocast=True)
    nat = _grad_stats(grads, ref, loss, ref_loss)
    yard = _grad_stats({k: ygrads[k] for k in grads}, ref, yloss, ref_loss)
    assert nat["n"] == yard["n"] and nat["n"] >= 0.95 * len(grads), (nat["n"], yard["n"], len(grads))
    print(f"{variant} 96 bf16 gradients vs the float64 oracle, {nat['n']} of {len(grads)} tensors (native | autocast-oracle yardstick):")
    failed = []
    for key, bound in BF16_BUDGET.items():
        cos = key in ("gcos", "worst_cos")
        ok = nat[key] >= bound if cos else nat[key] <= bound
        ok_y = (1.0 - nat[key]) <= 1.5 * (1.0 - yard[key]) if cos else nat[key] <= 1.5 * yard[key]
        name = f" ({nat['worst_cos_name']} | {yard['worst_cos_name']})" if key == "worst_cos" else ""
        print(f"  {key:9s} {nat[key]:.5g} | {yard[key]:.5g}   bound {bound:g}: {'within' if ok else 'OVER'}; 1.5 x yardstick: {'within' if ok_y else 'over'}{name}")
        if not (ok or ok_y):
            failed.append((key, nat[key], yard[key], bound))
    print("  largest per-tensor errors (max-abs, rel-L2, cosine):", [(k, round(e, 3), round(l2, 3), round(c, 4)) for e, l2, c, k in nat["errs"][:6]])
    assert not failed, failed


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("parts,B", [(2, 6), (3, 7)])
def test_train_forward_image_ranges(monkeypatch, dtype, parts, B):
    """model.image_ranges / lmv_block_fwd_range: the training forward of a stage's blocks as concurrent ranges of images (each on its own
    stream, one arena, whole-batch backward) against the one-call forward: logits, loss and every parameter gradient agree (fp32: to
    rounding -- the ranges only change the row counts the kernels see; bf16: the module budget), and two range runs give BIT-equal logits and loss (the
    ranges share nothing but read-only weights)."""
    import lemevit_amd.model as M
    img = det_tensor((B, 3, 96, 96), "ranges.img", 5).to(DEV)
    tgt = torch.arange(B, device=DEV) % 10

    def run(p):
        monkeypatch.setattr(M, "TRAIN_PARTS", p); monkeypatch.setattr(M, "TRAIN_PARTS_MIN_BATCH", 2)
        m = _model("lemevit_tiny", 10, 11, drop_path_rate=0.0).train()
        with torch.autocast("cuda", torch.bfloat16, enabled=dtype == torch.bfloat16):
            logits = m(img)
            loss = torch.nn.functional.cross_entropy(logits.float(), tgt)
        loss.backward()
        torch.cuda.synchronize()
        return logits.detach().float().cpu(), loss.item(), {k: v.grad.detach().float().cpu() for k, v in m.named_parameters() if v.grad is not None}

    l1, s1, g1 = run(1)
    l2, s2, g2 = run(parts)
    l3, s3, g3 = run(parts)
    assert torch.equal(l2, l3) and s2 == s3              # the forward pass is what the ranges change: bit-equal from run to run
    l0, s0, g0 = run(1)
    for k in g2:                                          # (the backward's split reductions use atomics: run-to-run noise with or without ranges)
        ref_noise = float((g0[k] - g1[k]).norm())
        assert float((g2[k] - g3[k]).norm()) <= max(4 * ref_noise, 1e-6 * float(g2[k].norm())), k
    tol = 2e-5 if dtype == torch.float32 else 2e-2
    close(l2, l1, tol, "logits")
    assert abs(s2 - s1) <= tol * max(1.0, abs(s1))
    assert g1.keys() == g2.keys()
    floor = 1e-3 * max(float(v.norm()) for v in g1.values())       # (a conv bias in front of a BatchNorm has a gradient of exactly-zero-plus-rounding)
    for k in g1:
        n1, dn = float(g1[k].norm()), float((g2[k] - g1[k]).norm())
        assert dn <= (2e-4 if dtype == torch.float32 else 5e-2) * max(n1, floor), (k, n1, dn)


def test_full_size_properties_bf16():
    """BASELINE-size run (Base, B=128, 224^2, bf16 autocast).  Size-independent properties of the hot path:
    every LeMeBlock is batch-independent -- permuting the batch permutes its outputs BIT-EXACTLY (checked per block with
    the library-conv boundary glue re-synchronised, because MIOpen's stride-2 conv is not position-invariant) -- the
    whole-model logits agree with a permuted and with a B=2 run to bf16 rounding, and one train step yields finite
    gradients for every parameter."""
    torch.manual_seed(0)
    m = L().create_model("lemevit_base", num_classes=1000, drop_path_rate=0.1).to(DEV).eval()
    B = 128
    x = torch.randn(B, 3, 224, 224, device=DEV)
    perm = torch.randperm(B, device=DEV)
    bf = torch.bfloat16
    with torch.no_grad(), torch.autocast("cuda", bf):
        a = m.downsample_layers[0](x.contiguous(memory_format=torch.channels_last))
        x1, H, W = m._to_tokens(a, bf)
        c1 = m.meta_token_downsample[0](m.meta_tokens.unsqueeze(0)).expand(B, -1, -1).to(bf).contiguous()
        for i in range(m.num_stages):
            if i > 0:
                if not isinstance(m.downsample_layers[i], torch.nn.Identity):
                    x1, H, W = m._to_tokens(m.downsample_layers[i](m._to_nchw(x1, H, W)), bf)
                c1 = m.meta_token_downsample[i](c1).to(bf).contiguous()
            x2, c2 = x1[perm].contiguous(), c1[perm].contiguous()
            for blk in m.stages[i]:
                x1, c1 = blk.forward_tokens(x1, c1, H, W)
                x2, c2 = blk.forward_tokens(x2, c2, H, W)
                assert torch.equal(x1[perm], x2) and torch.equal(c1[perm], c2), f"stage {i}: block output depends on batch position"
        y = m(x); yp = m(x[perm]); y2 = m(x[:2])
    scale = float(y.float().abs().max())
    assert float((y[perm].float() - yp.float()).abs().max()) <= 2e-2 * scale
    assert float((y[:2].float() - y2.float()).abs().max()) <= 2e-2 * scale
    m.train()
    with torch.autocast("cuda", bf):
        loss = torch.nn.functional.cross_entropy(m(x), torch.randint(0, 1000, (B,), device=DEV))
    loss.backward()
    assert torch.isfinite(loss)
    for k, p in m.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), k


def test_bf16_weight_copies_follow_fused_optimizer():
    """torch.optim.AdamW(fused=True) updates parameters in place WITHOUT bumping Tensor._version; the bf16 operand copies the
    kernels read must still be refreshed every training pass (and for the evaluation that follows)."""
    torch.manual_seed(0)
    m = L().create_model("lemevit_tiny", num_classes=10).to(DEV).train()
    opt = torch.optim.AdamW(m.parameters(), lr=5e-2, fused=True)
    x = torch.randn(4, 3, 64, 64, device=DEV)
    w = m.stages[2][0].mlp[0].weight
    from lemevit_amd.model import compute_copy
    outs = []
    for _ in range(3):
        opt.zero_grad(set_to_none=True)
        with torch.autocast("cuda", torch.bfloat16):
            out = m(x)
            out.float().square().mean().backward()
        assert torch.equal(compute_copy(w, torch.bfloat16), w.detach().to(torch.bfloat16)), "stale bf16 copy inside a training pass"
        opt.step()
        outs.append(out.detach().float().clone())
    assert float((outs[1] - outs[0]).abs().max()) > 0 and float((outs[2] - outs[1]).abs().max()) > 0, "the forward ignores optimizer updates"
    m.eval()
    with torch.no_grad(), torch.autocast("cuda", torch.bfloat16):
        m(x)
        assert torch.equal(compute_copy(w, torch.bfloat16), w.detach().to(torch.bfloat16)), "stale bf16 copy in evaluation after training"


def test_flat_adamw_matches_torch_adamw():
    """lemevit_amd.FlatAdamW (flat block parameters, gradients written in place by the block backward, one fused launch that
    also refreshes the bf16 operand copies) against torch.optim.AdamW on a twin model: same losses and parameters after 3
    bf16-autocast steps, and the bf16 copies equal the rounded parameters."""
    torch.manual_seed(0)
    Lm = L()
    m1 = Lm.create_model("lemevit_tiny", num_classes=10).to(DEV).train()
    m2 = Lm.create_model("lemevit_tiny", num_classes=10).to(DEV).train()
    m2.load_state_dict(m1.state_dict())
    decay = [p for n, p in m1.named_parameters() if p.ndim > 1]; plain = [p for n, p in m1.named_parameters() if p.ndim <= 1]
    o1 = torch.optim.AdamW([dict(params=decay, weight_decay=0.05), dict(params=plain, weight_decay=0.0)], lr=1e-3, eps=1e-8)
    o2 = Lm.FlatAdamW(m2, lr=1e-3, eps=1e-8, weight_decay=0.05)
    x = torch.randn(4, 3, 64, 64, device=DEV); y = torch.randint(0, 10, (4,), device=DEV)
    lf = torch.nn.CrossEntropyLoss()
    for step in range(3):
        losses = []
        for m, o in ((m1, o1), (m2, o2)):
            o.zero_grad(set_to_none=True)
            with torch.autocast("cuda", torch.bfloat16):
                loss = lf(m(x), y)
            loss.backward()
            o.step()
            losses.append(float(loss.detach()))
        assert abs(losses[0] - losses[1]) <= 2e-3 * max(1.0, abs(losses[0])), (step, losses)
    for (n, p1), (_, p2) in zip(m1.named_parameters(), m2.named_parameters()):
        d = float((p1 - p2).abs().max()); s = float(p1.abs().max()) + 1e-12
        # 3 Adam steps of lr 1e-3 move a weight by <= 3e-3; where the true gradient is ~0 (conv bias in front of BatchNorm) the
        # SIGN of the update is rounding noise, so two correct implementations may differ by twice that
        assert d <= 5e-3 * s + 6.5e-3, f"{n}: {d:.3e} vs scale {s:.3e}"
    w = m2.stages[2][0].mlp[0].weight
    assert torch.equal(w._lmv_shadow, w.detach().to(torch.bfloat16))
    sd = m1.state_dict()
    m2.load_state_dict(sd)                                   # post-hook refreshes the bf16 copies
    assert torch.equal(w._lmv_shadow, w.detach().to(torch.bfloat16))


def test_flat_grad_sync_single_rank_nccl():
    """FlatGradSync over RCCL with a 1-rank process group: the chunked asynchronous all-reduces hooked into the block backward,
    the flattened exchange of the remaining gradients and the buffer broadcast must leave a training step unchanged."""
    import os
    import torch.distributed as dist
    from lemevit_amd.dist import attach_flat_grad_sync
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1"); os.environ.setdefault("MASTER_PORT", "29541")
    created = not dist.is_initialized()
    if created:
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device(DEV))
    try:
        torch.manual_seed(0)
        Lm = L()
        m1 = Lm.create_model("lemevit_tiny", num_classes=10).to(DEV).train()
        m2 = Lm.create_model("lemevit_tiny", num_classes=10).to(DEV).train()
        m2.load_state_dict(m1.state_dict())
        o1 = Lm.FlatAdamW(m1, lr=1e-3, weight_decay=0.05); o2 = Lm.FlatAdamW(m2, lr=1e-3, weight_decay=0.05)
        sync = attach_flat_grad_sync(m2, o2, nchunks=3, force=True)
        assert sync.active and len(sync.bounds) == 3 and sync.bounds[0][0] == 0 and sync.bounds[-1][1] == o2._flat_g.numel()
        x = torch.randn(4, 3, 64, 64, device=DEV); y = torch.randint(0, 10, (4,), device=DEV)
        for _ in range(2):
            for m, o, s in ((m1, o1, None), (m2, o2, sync)):
                torch.manual_seed(7)                       # same DropPath draws for both twins
                o.zero_grad()
                if s is not None:
                    s.broadcast_buffers(m)
                with torch.autocast("cuda", torch.bfloat16):
                    loss = torch.nn.functional.cross_entropy(m(x), y)
                loss.backward()
                if s is not None:
                    assert len(s._work) >= 1, "no chunk was released during the backward pass"
                    s.finish()
                o.step()
        # every kernel of the step is ours and reduces in a fixed order (round 2: the stem / stage-transition convolutions left MIOpen,
        # whose weight gradients differed from run to run): the twins must agree BIT FOR BIT on every parameter of every stage
        for (n, p1), (_, p2) in zip(m1.named_parameters(), m2.named_parameters()):
            assert torch.equal(p1, p2), (n, float((p1 - p2).abs().max()))
    finally:
        if created:
            dist.destroy_process_group()


def test_flat_adamw_checkpoint_resume_is_bit_identical(tmp_path):
    """Checkpoint / resume (the reference: timm's CheckpointSaver + resume_checkpoint, main.py:300-312): model.state_dict() + FlatAdamW.state_dict() saved with torch.save after two
    steps and loaded into a FRESH model and optimizer must continue exactly like the uninterrupted run -- parameters, BatchNorm statistics, both moments, the step count (bias
    correction) and the bf16 operand copies the kernels read."""
    Lm = L()

    def make():
        torch.manual_seed(0)
        m = Lm.create_model("lemevit_tiny", num_classes=10, drop_path_rate=0.1).to(DEV).train()
        return m, Lm.FlatAdamW(m, lr=1e-3, weight_decay=0.05)

    x = torch.randn(4, 3, 64, 64, device=DEV); y = torch.randint(0, 10, (4,), device=DEV)

    def steps(m, o, first, n):
        for i in range(first, first + n):
            torch.manual_seed(100 + i)                  # DropPath draws of step i
            o.zero_grad(set_to_none=False)
            with torch.autocast("cuda", torch.bfloat16):
                loss = torch.nn.functional.cross_entropy(m(x), y)
            loss.backward(); o.step()

    m1, o1 = make(); steps(m1, o1, 0, 4)
    m2, o2 = make(); steps(m2, o2, 0, 2)
    path = tmp_path / "ckpt.pt"
    torch.save({"model": m2.state_dict(), "opt": o2.state_dict()}, path)
    del m2, o2
    torch.manual_seed(12345)                            # a different initialisation: everything must come from the file
    m3 = Lm.create_model("lemevit_tiny", num_classes=10, drop_path_rate=0.1).to(DEV).train()
    o3 = Lm.FlatAdamW(m3, lr=1e-3, weight_decay=0.05)
    ck = torch.load(path, map_location=DEV)
    m3.load_state_dict(ck["model"]); o3.load_state_dict(ck["opt"])
    steps(m3, o3, 2, 2)
    torch.cuda.synchronize()
    for (k, a), (_, b) in zip(m1.state_dict().items(), m3.state_dict().items()):
        assert torch.equal(a, b), (k, float((a.float() - b.float()).abs().max()))
    assert torch.equal(o1._exp_avg, o3._exp_avg) and torch.equal(o1._exp_avg_sq, o3._exp_avg_sq) and torch.equal(o1._shadow, o3._shadow)
    assert int(o1._step_dev.item()) == int(o3._step_dev.item()) == 4


# ------------------------------------------------------------------------------------------------
# dense-prediction backbone
def _backbone(cfg, seed):
    from lemevit_amd.model import LeMeViTBackbone
    m = LeMeViTBackbone(**cfg)
    spec = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    m.load_state_dict(fill_state_dict(spec, seed))
    return m.to(DEV)


@pytest.mark.parametrize("name", ["dense_tiny_224", "dense_tiny_160x96"])
def test_dense_backbone_forward(golden, name):
    """Multi-scale feature maps of the detection / segmentation backbone vs the reference's own backbone file (fp32 1e-5, bf16 autocast 2e-2)."""
    meta, g = golden(name)
    m = _backbone(meta["cfg"], meta["seed"]).eval()
    assert len(m.state_dict()) == meta["nkeys"]
    img = det_tensor((meta["B"], 3, meta["H"], meta["W"]), name + ".img", 6).to(DEV)
    with torch.no_grad():
        outs = m(img)
    assert [list(o.shape) for o in outs] == meta["shapes"]
    for i, o in enumerate(outs):
        close(sample(o.flatten(2).transpose(1, 2).contiguous(), 8192), g[f"out{i}"], 1e-5, f"{name}.out{i}")
    with torch.no_grad(), torch.autocast("cuda", torch.bfloat16):
        outs = m(img)
    for i, o in enumerate(outs):
        close(sample(o.float().flatten(2).transpose(1, 2).contiguous(), 8192), g[f"out{i}"], 2e-2, f"{name}.out{i} bf16")


def test_dense_block_backward_fp32(golden):
    """The dense S block: c passes through (bit-identical) and every gradient matches the reference."""
    meta, g = golden("blockgrad_Sx")
    C, h, H, W, B = meta["C"], meta["h"], meta["H"], meta["W"], meta["B"]
    blk = L().LeMeBlock(dim=C, attn_drop=0.0, proj_drop=0.0, drop_path=0.0, attn_type="S", num_heads=h, dense=True)
    m = load(blk, "blk.", meta["seed"]).eval()
    x = det_tensor((B, C, H, W), "blockgrad_Sx.x", 3).to(DEV).requires_grad_(True); c = det_tensor((B, 16, C), "blockgrad_Sx.c", 3).to(DEV).requires_grad_(True)
    gx = det_tensor((B, C, H, W), "blockgrad_Sx.gx", 3).to(DEV); gc = det_tensor((B, 16, C), "blockgrad_Sx.gc", 3).to(DEV)
    xo, co = m(x, c)
    ((xo * gx).sum() + (co * gc).sum()).backward()
    close(xo, g["x_out"], 1e-5, "x_out")
    assert torch.equal(co.detach(), c.detach()) and torch.equal(c.grad, gc)
    close(x.grad, g["dx"], 2e-5, "dx")
    for k, p in m.named_parameters():
        ref = g["grad." + k]
        if np.abs(ref).max() == 0:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0
        else:
            close(p.grad, ref, 3e-5, "grad " + k)


def test_dense_backbone_train_step_bf16():
    """Train-mode pass of the dense backbone (frozen norm layers as the reference's train()): finite multi-scale outputs and gradients,
    meta-token gradient reaches `meta_tokens` only through the C / D stages."""
    cfg = dict(depth=[1, 1, 1, 2, 1], embed_dim=[64, 64, 128, 192, 320], head_dim=32, mlp_ratios=[4, 4, 4, 4, 4], attn_type=["C", "D", "D", "S", "S"],
               queries_len=16, drop_path_rate=0.1)
    m = _backbone(cfg, 3).train()
    assert not any(mod.training for mod in m.modules() if isinstance(mod, (torch.nn.BatchNorm2d, torch.nn.LayerNorm)))
    img = det_tensor((2, 3, 96, 128), "dense.train.img", 6).to(DEV)
    with torch.autocast("cuda", torch.bfloat16):
        outs = m(img)
        sum(o.float().square().mean() for o in outs).backward()
    assert [tuple(o.shape) for o in outs] == [(2, 64, 24, 32), (2, 128, 12, 16), (2, 192, 6, 8), (2, 320, 3, 4)]
    for k, p in m.named_parameters():
        if k.startswith(("extra_norms", "norm.", "norm_c.")):
            assert p.grad is None
        else:
            assert p.grad is not None and torch.isfinite(p.grad).all(), k


# ------------------------------------------------------------------------------------------------
# round-2 regressions
def test_eval_fold_follows_training_step():
    """eval -> train step -> eval: the conv+BN fold made by the first evaluation must not survive the training step.  The native
    BatchNorm kernel writes the running statistics through raw pointers and fused optimizers update weights in place, both WITHOUT
    bumping Tensor._version, so a version-keyed fold would silently feed stale stem weights / statistics to validation."""
    torch.manual_seed(0)
    Lm = L()
    m = Lm.create_model("lemevit_tiny", num_classes=10).to(DEV)
    opt = Lm.FlatAdamW(m, lr=5e-2, weight_decay=0.05)
    x = torch.randn(4, 3, 64, 64, device=DEV); y = torch.randint(0, 10, (4,), device=DEV)
    m.eval()
    with torch.no_grad():
        first = m(x).clone()
    m.train()
    for _ in range(2):
        opt.zero_grad()
        torch.nn.functional.cross_entropy(m(x), y).backward()
        opt.step()
    m.eval()
    with torch.no_grad():
        folded = m(x)
    unfolded = m(x).detach()               # grad enabled: conv and BatchNorm run separately from the live tensors
    assert float((folded - first).abs().max()) > 1e-4, "evaluation ignores the training steps"
    close(folded, unfolded.cpu().numpy(), 1e-5, "fold after training")


def test_flat_adamw_survives_model_zero_grad():
    """model.zero_grad() (set_to_none=True) detaches p.grad from the flat gradient buffer; FlatAdamW must re-bind (and keep a
    gradient autograd allocated meanwhile) instead of silently stepping on zeros.  param_groups[0] lists the flat parameters."""
    torch.manual_seed(0)
    Lm = L()
    m1 = Lm.create_model("lemevit_tiny", num_classes=10).to(DEV).train()
    m2 = Lm.create_model("lemevit_tiny", num_classes=10).to(DEV).train()
    m2.load_state_dict(m1.state_dict())
    o1 = Lm.FlatAdamW(m1, lr=1e-3, weight_decay=0.05); o2 = Lm.FlatAdamW(m2, lr=1e-3, weight_decay=0.05)
    assert len(o2.param_groups[0]["params"]) == len(o2._slices) > 0
    x = torch.randn(4, 3, 64, 64, device=DEV); y = torch.randint(0, 10, (4,), device=DEV)
    w0 = m1.stages[3][0].mlp[0].weight.detach().clone()
    for m, o, hostile in ((m1, o1, False), (m2, o2, True)):
        torch.manual_seed(7)
        if hostile:
            m.zero_grad(set_to_none=True)          # every p.grad is None now: the backward goes through autograd's accumulation
        else:
            o.zero_grad()
        torch.nn.functional.cross_entropy(m(x), y).backward()
        o.step()
    w1, w2 = m1.stages[3][0].mlp[0].weight, m2.stages[3][0].mlp[0].weight
    assert float((w1 - w0).abs().max()) > 1e-4, "the reference twin did not train"
    assert float((w2 - w0).abs().max()) > 1e-4, "FlatAdamW stepped on zeros after model.zero_grad()"
    # the flat gradient buffers still hold this step's gradients: the stray autograd gradients were copied in before the update
    i = [p is w2 for _, p, _, _ in o2._slices].index(True)
    _, _, off, n = o2._slices[i]
    g1, g2 = o1._flat_g[off:off + n], o2._flat_g[off:off + n]
    assert float(g1.abs().max()) > 0 and torch.allclose(g1, g2, rtol=1e-4, atol=1e-6 * float(g1.abs().max())), float((g1 - g2).abs().max())
    # (weights: an Adam step moves every entry by ~lr whatever the gradient's size, so entries whose gradient is rounding noise may differ by 2 lr)
    assert float((w1 - w2).abs().max()) <= 2.5e-3 and float((w1 - w2).abs().mean()) <= 1e-5
    assert w2.grad is o2._grad_views[i]


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two MI355X (BASELINE config 4 runs on an 8-GPU node; the 1-GPU boxes take the gloo form below)")
@pytest.mark.parametrize("compress", [None, "bf16"])
def test_two_rank_gradients_equal_single_process_rccl(tmp_path, compress):
    """The same check over RCCL / xGMI with one device per rank (main.py:333, scripts/train.sh:3-8): lights up on any box with >= 2 GPUs."""
    _two_rank_vs_single(tmp_path, compress, "nccl")


@pytest.mark.parametrize("compress", [None, "bf16"])
def test_two_rank_gradients_equal_single_process(tmp_path, compress):
    _two_rank_vs_single(tmp_path, compress, "gloo")


def _two_rank_vs_single(tmp_path, compress, backend):
    """SURVEY section 4 "Distributed", on the PRODUCT model: lemevit_tiny (fp32 kernels) trained by two ranks that share this GPU
    (gloo process group), FlatAdamW + FlatGradSync, global batch 8 split 4 + 4, against one process on the whole batch.
    LayerNorm / attention / MLP are per-sample, so block gradients must agree to fp32 rounding; the stem and stage-transition
    BatchNorms use per-rank batch statistics exactly as the reference's DDP default (main.py:222-234, no SyncBN), so parameters
    upstream of a BatchNorm would differ by design -- so the BatchNorms are put in eval mode (fixed statistics) on both sides and
    EVERY parameter gradient is compared."""
    import socket
    import torch.multiprocessing as mp
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    out = str(tmp_path / "g2.pt")
    mp.spawn(_two_rank_worker_bn_eval, args=(2, port, out, compress, backend), nprocs=2, join=True)
    got = torch.load(out)
    Lm = L()
    torch.manual_seed(0)
    m = Lm.create_model("lemevit_tiny", num_classes=10, drop_path_rate=0.0).to(DEV).train()
    for mod in m.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.eval()
    opt = Lm.FlatAdamW(m, lr=1e-3, weight_decay=0.05)
    torch.manual_seed(1)
    x = torch.randn(8, 3, 64, 64, device=DEV); y = torch.randint(0, 10, (8,), device=DEV)
    opt.zero_grad()
    torch.nn.functional.cross_entropy(m(x), y).backward()
    tol = 1e-2 if compress else 2e-5
    checked = 0
    for n, p in m.named_parameters():
        if p.grad is None:
            continue
        ref = p.grad.detach().float().cpu()
        # the mean over two half-batch gradients equals the full-batch gradient (CrossEntropyLoss averages over the batch)
        err = float((got[n] - ref).abs().max()); scale = float(ref.abs().max()) + 1e-12
        assert err <= tol * scale + 1e-7, f"{n}: {err:.3e} vs scale {scale:.3e}"
        checked += 1
    assert checked > 100


def _two_rank_worker_bn_eval(rank, world, port, out, compress, backend="gloo"):
    import os
    local = rank if backend == "nccl" else 0               # RCCL wants one device per rank; gloo lets both ranks share cuda:0 (1-GPU boxes)
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(local), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    import torch.distributed as dist
    torch.cuda.set_device(local)
    DEV = f"cuda:{local}"
    if backend == "nccl":
        dist.init_process_group("nccl", device_id=torch.device(DEV))
    else:
        dist.init_process_group("gloo")
    import lemevit_amd as Lm
    from lemevit_amd.dist import attach_flat_grad_sync, shard_batch
    torch.manual_seed(0)
    m = Lm.create_model("lemevit_tiny", num_classes=10, drop_path_rate=0.0).to(DEV).train()
    for mod in m.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.eval()                                   # fixed statistics: every remaining op is per-sample
    opt = Lm.FlatAdamW(m, lr=1e-3, weight_decay=0.05)
    sync = attach_flat_grad_sync(m, opt, nchunks=3, compress=compress)
    torch.manual_seed(1)
    x = torch.randn(8, 3, 64, 64, device=DEV); y = torch.randint(0, 10, (8,), device=DEV)
    idx = list(shard_batch(8, rank, world))
    opt.zero_grad()
    torch.nn.functional.cross_entropy(m(x[idx]), y[idx]).backward()
    sync.finish()
    if rank == 0:
        torch.save({n: p.grad.detach().float().cpu() for n, p in m.named_parameters() if p.grad is not None}, out)
    dist.destroy_process_group()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("kind,C,h,Hs", [("S", 192, 6, 7), ("D", 96, 3, 14), ("C", 64, 2, 14)])
def test_native_block_schedule_equals_python_schedule(monkeypatch, kind, C, h, Hs, dtype):
    """lmv_block_fwd / lmv_block_bwd (csrc/block.hip) run the SAME kernels in the same order as lemevit_amd/blocks.py: outputs, input
    gradients and every parameter gradient must be bit-identical -- with DropPath scale vectors on all four branches and the weight
    gradients on the side stream.  (Parity of either schedule with the reference: test_block_backward_*.)"""
    _native_vs_python(monkeypatch, kind, C, h, Hs, dtype, 5)


@pytest.mark.parametrize("kind,C,h,Hs", [("S", 384, 12, 14), ("D", 96, 3, 56)])
def test_native_block_schedule_equals_python_schedule_full_size(monkeypatch, kind, C, h, Hs):
    """The same bit-equality at the FULL Base shapes of config 3 (B = 128: stage 3 = 196 + 16 tokens x 384, stage 1 = 3136 + 16 tokens x 96):
    arena / scratch layouts, split-K plans and 32-bit index arithmetic only show their bugs at size."""
    _native_vs_python(monkeypatch, kind, C, h, Hs, torch.bfloat16, 128)


def _native_vs_python(monkeypatch, kind, C, h, Hs, dtype, B):
    import lemevit_amd.model as M
    from lemevit_amd.blocks import PARAM_NAMES
    N, Mt = Hs * Hs, 16
    names = PARAM_NAMES[kind]
    blk = load(_block(kind, C, h), "blk.", 11)
    allp = dict(blk.named_parameters())
    params = {n: allp[n] for n in names}
    nm = 2 if kind == "C" else 4
    masks = tuple((det_tensor((B,), f"mask{i}", 4).abs() > 0.3).float().to(DEV) / 0.7 for i in range(nm))
    res = {}
    for native in (True, False):
        monkeypatch.setattr(M, "_NATIVE", native)
        for p in params.values():
            p.grad = None
        x = det_tensor((B, N, C), "x", 6).to(DEV, dtype).requires_grad_(True); c = det_tensor((B, Mt, C), "c", 6).to(DEV, dtype).requires_grad_(True)
        gx = det_tensor((B, N, C), "gx", 6).to(DEV, dtype); gc = det_tensor((B, Mt, C), "gc", 6).to(DEV, dtype)
        xo, co = M.run_block(kind, x, c, Hs, Hs, params, masks)
        ((xo.float() * gx.float()).sum() + (co.float() * gc.float()).sum()).backward()
        torch.cuda.synchronize()
        res[native] = [xo.detach().clone(), co.detach().clone(), x.grad.clone(), c.grad.clone()] + [p.grad.clone() for p in params.values()]
        monkeypatch.setattr(M, "_FUSED", False)
        with torch.no_grad():                 # the no-grad (inference) entry of the same schedule
            xe, ce = M.run_block(kind, x.detach(), c.detach(), Hs, Hs, params, masks)
        assert torch.equal(xe, xo.detach()) and torch.equal(ce, co.detach())
        monkeypatch.setattr(M, "_FUSED", True)
        with torch.no_grad():                 # ... and its fused form (bf16: LayerNorm folded into the projections, one-kernel MLP half; DropPath scales included)
            xf, cf = M.run_block(kind, x.detach(), c.detach(), Hs, Hs, params, masks)
        if dtype == torch.float32:
            assert torch.equal(xf, xe) and torch.equal(cf, ce)          # the fused path is bf16 only
        else:
            for a, b, what in ((xf, xe, "x"), (cf, ce, "c")):
                err = float((a.float() - b.float()).abs().max()) / float(b.float().abs().max())
                assert err <= 2e-2, f"{kind} fused inference {what}: {err:.2e}"
    labels = ["x_out", "c_out", "dx", "dc"] + ["grad " + n for n in names]
    for a, b, what in zip(res[True], res[False], labels):
        assert torch.equal(a, b), f"{kind} {dtype} {what}: native and Python schedules differ by {float((a.float() - b.float()).abs().max()):.3e}"


def test_block_bwd_two_threads_two_streams():
    """include/lemevit_hip.h promises a stateless, re-entrant library: two host threads run lmv_block_bwd (raw C ABI) on the SAME device at the
    same time, each on its own main + side stream, 12 rounds -- every output and every parameter gradient must be bit-identical to the
    one-thread run.  (Round 2 shared ONE fork / join event pair per device between all calls: thread A's side stream could then wait on the
    record thread B had just made; csrc/block.hip now hands every call its own pair.)"""
    import threading
    import lemevit_amd.model as M
    from lemevit_amd import ops
    from lemevit_amd._lib import lib, check
    from lemevit_amd.blocks import PARAM_NAMES
    kind, C, h, Hs, B, Mt = "S", 192, 6, 14, 16, 16
    N = Hs * Hs
    names = PARAM_NAMES[kind]
    dtype = torch.bfloat16
    probs = []
    for i in range(2):
        blk = load(_block(kind, C, h), "blk.", 21 + i)
        allp = dict(blk.named_parameters())
        P = {n: M.compute_copy(allp[n], dtype if M._is_matrix(n) else torch.float32).contiguous() for n in names}
        masks = tuple((det_tensor((B,), f"tmask{i}{q}", 4).abs() > 0.3).float().to(DEV) / 0.7 for q in range(4))
        main, side = torch.cuda.Stream(), torch.cuda.Stream()
        x = det_tensor((B, N, C), f"tx{i}", 6).to(DEV, dtype); c = det_tensor((B, Mt, C), f"tc{i}", 6).to(DEV, dtype)
        gx = det_tensor((B, N, C), f"tgx{i}", 6).to(DEV, dtype); gc = det_tensor((B, Mt, C), f"tgc{i}", 6).to(DEV, dtype)
        torch.cuda.synchronize()
        with torch.cuda.stream(main):
            xo, co, (d, arena) = M.native_block_forward(kind, x, c, Hs, Hs, names, P, masks, save=True)
        nb = M._sized(lib.lmv_block_bwd_scratch_bytes, d, kind, x, c, Hs, Hs)
        scratch = torch.empty(nb + 4096, device=DEV, dtype=torch.uint8)
        G = {n: torch.zeros(P[n].shape, device=DEV, dtype=torch.float32) for n in names}
        M._fill_ptrs(d, kind, names, G, "g_")
        d.flags = 0
        probs.append(dict(d=d, arena=arena, x=x, c=c, gx=gx, gc=gc, dx=torch.empty_like(x), dc=torch.empty_like(c), scratch=scratch, G=G, main=main, side=side, P=P, masks=masks))
    torch.cuda.synchronize()

    def run(p, rounds):
        torch.cuda.set_device(0)
        for _ in range(rounds):
            for g in p["G"].values():
                with torch.cuda.stream(p["main"]):
                    g.zero_()
            check(lib.lmv_block_bwd(p["d"], p["x"].data_ptr(), p["c"].data_ptr(), p["arena"].data_ptr(), p["arena"].numel(), p["gx"].data_ptr(), p["gc"].data_ptr(),
                                    p["dx"].data_ptr(), p["dc"].data_ptr(), p["scratch"].data_ptr(), p["scratch"].numel(), p["main"].cuda_stream, p["side"].cuda_stream),
                  "lmv_block_bwd")
        p["main"].synchronize(); p["side"].synchronize()

    ref = []
    for p in probs:                       # one thread, one problem at a time
        run(p, 1)
        torch.cuda.synchronize()
        ref.append([p["dx"].clone(), p["dc"].clone()] + [p["G"][n].clone() for n in names])
    errs = []

    def worker(p):
        try:
            run(p, 12)
        except Exception as e:            # pragma: no cover
            errs.append(e)

    th = [threading.Thread(target=worker, args=(p,)) for p in probs]
    for t in th:
        t.start()
    for t in th:
        t.join()
    torch.cuda.synchronize()
    assert not errs, errs
    for i, p in enumerate(probs):
        got = [p["dx"], p["dc"]] + [p["G"][n] for n in names]
        for a, b, what in zip(got, ref[i], ["dx", "dc"] + ["grad " + n for n in names]):
            assert torch.equal(a, b), f"problem {i} {what}: threaded run differs from the serial one by {float((a.float() - b.float()).abs().max()):.3e}"
