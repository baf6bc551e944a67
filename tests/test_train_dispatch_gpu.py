"""The size-gated kernels of a training step, run the way a training step runs them, against the float64 oracle.

A block chooses its kernels by row count and by whether FlatAdamW keeps transposed bf16 weight copies: the register-stationary GEMM (csrc/rsgemm.hip, taken by
itself from 8192 rows: fc1 + GELU + pre-activation copy, qkv at K = 192, the GELU' dX of fc2 through fc2_wt), the whole-width GEMM (csrc/wngemm.hip, residual
epilogues between 16384 and 32768 rows: proj, fc2), lmv_linear_res_ln_fwd (proj + residual + norm2), lmv_linear_dx_ln_bwd (dX + LayerNorm backward: the same window,
C = 384 and a transposed copy, which only FlatAdamW gives a trainable block) and, in the fused inference schedule, mlp_split384 (16384 .. 65536 rows).  The other
block tests stay at <= 636 rows or run without FlatAdamW, and the kernel-level tests force the kernels on at <= 4149 rows, so none of them reaches these choices as
a block makes them.  Here every case is the smallest batch that reaches its leaf (rows = B * (Hs * Hs + 16)):

    S 384 B = 3     636 rows   transposed-copy dX on the tile kernel for a trainable block, gradients accumulated in place into the flat buffer
    S 192 B = 39   8268 rows   rs alone at K = 192: fc1, qkv, fc2 dX
    D 192 B = 11   8800 rows   rs alone with two problems that have their own weights (qkv1 / qkv2); only fc2_wt
    S 384 B = 39   8268 rows   rs alone at K = 384, below the wn window
    S 384 B = 78  16536 rows   lower edge of the window: wn proj and fc2, res_ln_fwd, dx_ln_bwd twice
    S 384 B = 154 32648 rows   upper edge: 236 + 20 = 256 panels, one per CU
    S 384 B = 77 / 155         16324 / 32860 rows: just outside the window (launch kinds only)

Reference: oracle.leme_block in float64 with autograd on the bf16-rounded matrices, the fp32 vectors and the same bf16-rounded x, c, gx, gc and DropPath scale
vectors.  Tolerances: the bf16 block budget of tests/test_model_gpu.py::test_block_backward_bf16_vs_oracle, 2e-2 of max-abs for outputs and 3e-2 for every gradient.
Whether that budget holds at these row counts is measured next to it by a YARDSTICK on the same inputs: the kernels the suite already checks (gemm_rs = 0,
gemm_wn = 0, no FlatAdamW, the batch in chunks of at most 77 images so that no chunk enters the window; images do not interact inside a block, so the chunk outputs
are concatenated and autograd sums the parameter gradients).  The production run may be at most 1.5 x the yardstick's error against the oracle on x_out, c_out, dx,
dc and on the relative L2 error of all parameter gradients concatenated (1.5: the margin test_mlp_dx_fused_kernel gives a re-fused form of the same arithmetic;
both sides round activations to bf16 at the same points, except that the fused dX + LayerNorm backward keeps dy in fp32).  A tensor on which the yardstick itself
is over the budget would be bound by 1.5 x the yardstick instead; on the MI355X none was (the figures are in test_production_block_vs_oracle's docstring).

The launch kinds of the library's timing probe (lmv_debug_launch_timing) are the evidence of which kernel ran: 8 = register-stationary GEMM, 9 = whole-width GEMM
incl. res_ln_fwd / dx_ln_bwd, 0 = tile kernel in forward form, 4 = dX, 5 = dW, 11 = exact LayerNorm + Linear.  profiles/train_dispatch_coverage.txt holds the kinds
a run of this file launched per case (the "dispatch ..." lines it prints)."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from detfill import det_tensor, fill_state_dict
from oracle import lemevit_oracle as O

DEV = "cuda:0"
SEED = 5
MT = 16                    # meta tokens
CHUNK = 77                 # images per yardstick chunk: 77 * 212 = 16324 rows, below the whole-width window
OUT_TOL, GRAD_TOL, MARGIN = 2e-2, 3e-2, 1.5


def L():
    import lemevit_amd
    return lemevit_amd


def Mod():
    import lemevit_amd.model as M
    return M


def close(out, ref, tol, what):
    out = np.asarray(out.detach().float().cpu().numpy() if torch.is_tensor(out) else out, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    assert out.shape == ref.shape, (what, out.shape, ref.shape)
    assert np.isfinite(out).all(), what
    mx = max(np.abs(ref).max(), 1e-30)
    err = np.abs(out - ref).max()
    print(f"{what}: max-abs err {err / mx:.2e} of max-abs")
    assert err <= tol * mx, f"{what}: max-abs err {err:.3e} > {tol:.0e} * {mx:.3e}"
    return err / mx


def load(module, prefix, seed):
    spec = {prefix + k: tuple(v.shape) for k, v in module.state_dict().items()}
    sd = fill_state_dict(spec, seed)
    module.load_state_dict({k[len(prefix):]: v for k, v in sd.items()})
    return module.to(DEV)


def _block(t, C, h):
    return L().LeMeBlock(dim=C, attn_drop=0.0, proj_drop=0.0, drop_path=0.0, attn_type=t, num_heads=h)


@pytest.fixture
def cfg():
    """lmv_config_set for the test, restored afterwards."""
    from lemevit_amd import _lib
    saved = {}

    def set_(key, value):
        saved.setdefault(key, _lib.config_get(key))
        _lib.config_set(key, value)
    yield set_
    for k, v in saved.items():
        _lib.config_set(k, v)


class _Kinds:
    """The launch kinds the library's timing probe saw (lmv_debug_launch_timing), in the order the host issued them."""

    def __enter__(self):
        from lemevit_amd import _lib
        self.lib, self.cap = _lib.lib, 4096
        _lib.check(self.lib.lmv_debug_launch_timing(self.cap), "lmv_debug_launch_timing")
        return self

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        ms = (ctypes.c_float * self.cap)(); fl = (ctypes.c_double * self.cap)(); by = (ctypes.c_double * self.cap)(); kd = (ctypes.c_int * self.cap)()
        n = self.lib.lmv_debug_launch_timing_read(ms, fl, by, kd, self.cap)
        self.kinds = [kd[i] for i in range(n)]
        self.lib.lmv_debug_launch_timing(0)
        return False


def _report(what, case, kinds):
    kind, C, h, Hs, B = case
    print(f"dispatch {what} {kind} C={C} Hs={Hs} B={B} rows={B * (Hs * Hs + MT)}: " + " ".join(str(k) for k in kinds))


# ------------------------------------------------------------------------------------------------
# inputs and the float64 reference: built once per case, shared by the tests, never modified
_INPUTS: dict = {}
_ORACLE: dict = {}


def _inputs(case):
    """bf16-rounded x, c, gx, gc (token-major) and the DropPath scale vectors of tests/test_model_gpu.py::_native_vs_python, on the host."""
    if case not in _INPUTS:
        kind, C, h, Hs, B = case
        N = Hs * Hs
        bf = lambda shape, name: det_tensor(shape, name, 6).to(torch.bfloat16)
        nm = 2 if kind == "C" else 4
        masks = tuple((det_tensor((B,), f"mask{i}", 4).abs() > 0.3).float() / 0.7 for i in range(nm))
        _INPUTS[case] = dict(x=bf((B, N, C), "x"), c=bf((B, MT, C), "c"), gx=bf((B, N, C), "gx"), gc=bf((B, MT, C), "gc"), masks=masks)
    return _INPUTS[case]


def _oracle_sd(kind, C, h, grad):
    """What load(_block(kind, C, h), "blk.", SEED) holds, as the kernels read it: the matrices rounded to bf16, the vectors in fp32, all cast to double."""
    spec = {"blk." + k: tuple(v.shape) for k, v in _block(kind, C, h).state_dict().items()}
    sd = {}
    for k, v in fill_state_dict(spec, SEED).items():
        v = v.to(torch.bfloat16).double() if ("attn." in k or "mlp." in k) and k.endswith("weight") else v.double()
        sd[k] = v.requires_grad_(grad)
    return sd


def _oracle(case, grad=True):
    """x_out, c_out (and with grad: dx, dc, every parameter gradient) of oracle.leme_block in float64, as numpy arrays."""
    hit = _ORACLE.get(case)
    if hit is not None and (not grad or "dx" in hit):
        return hit
    kind, C, h, Hs, B = case
    inp = _inputs(case)
    sd = _oracle_sd(kind, C, h, grad)
    x = inp["x"].double().requires_grad_(grad); c = inp["c"].double().requires_grad_(grad)
    masks = [m.double() for m in inp["masks"]]
    with torch.set_grad_enabled(grad):
        xo, co = O.leme_block(sd, "blk.", kind, x, c, Hs, Hs, h, masks)
        res = dict(x_out=xo.detach().numpy(), c_out=co.detach().numpy())
        if grad:
            ((xo * inp["gx"].double()).sum() + (co * inp["gc"].double()).sum()).backward()
            res.update(dx=x.grad.numpy(), dc=c.grad.numpy(), grads={k[4:]: v.grad.numpy() for k, v in sd.items() if v.grad is not None})
    _ORACLE[case] = res
    return res


# ------------------------------------------------------------------------------------------------
# the two sides
def _run(case, flat, i0=0, i1=None, blk=None, probe=True):
    """One block forward + backward over the images [i0, i1) through model.run_block, the way a training step runs it.  flat: FlatAdamW on the lone block first
    (bf16 shadows, transposed copies, in-place flat .grad views).  Returns x_out, c_out, dx, dc, the block (parameter gradients in p.grad) and the launch kinds."""
    from lemevit_amd import blocks
    from lemevit_amd.blocks import PARAM_NAMES
    M = Mod()
    kind, C, h, Hs, B = case
    inp = _inputs(case)
    i1 = B if i1 is None else i1
    opt = None
    if blk is None:
        blk = load(_block(kind, C, h), "blk.", SEED)
        if flat:
            opt = L().FlatAdamW(blk)
            opt.zero_grad()
    allp = dict(blk.named_parameters())
    params = {n: allp[n] for n in PARAM_NAMES[kind]}
    masks = tuple(m[i0:i1].contiguous().to(DEV) for m in inp["masks"])
    x = inp["x"][i0:i1].to(DEV).requires_grad_(True); c = inp["c"][i0:i1].to(DEV).requires_grad_(True)
    gx = inp["gx"][i0:i1].to(DEV); gc = inp["gc"][i0:i1].to(DEV)
    torch.cuda.synchronize()
    with _Kinds() as k:
        xo, co = M.run_block(kind, x, c, Hs, Hs, params, masks)
        ((xo.float() * gx.float()).sum() + (co.float() * gc.float()).sum()).backward()
        blocks.drain_deferred()              # what FlatAdamW.step does first: the weight-gradient side stream is joined before anything reads the gradients
        torch.cuda.synchronize()
    if opt is not None:                      # the kernels accumulated straight into the flat buffer: every .grad is still the optimizer's view of it
        assert all(p.grad is v for (_, p, _, _), v in zip(opt._slices, opt._grad_views))
        assert getattr(allp["mlp.3.weight"], "_lmv_shadow_t", None) is not None          # ... and the fc2 dX reads a transposed copy
    return dict(x_out=xo.detach(), c_out=co.detach(), dx=x.grad, dc=c.grad, blk=blk, opt=opt, kinds=k.kinds)


def _yardstick(case, cfg):
    """The kernels the suite already checks, on the same inputs: rs / wn off, no FlatAdamW, chunks of at most CHUNK images."""
    cfg("gemm_rs", 0); cfg("gemm_wn", 0)
    B = case[4]
    parts, blk, kinds = [], None, []
    for i0 in range(0, B, CHUNK):
        r = _run(case, False, i0, min(B, i0 + CHUNK), blk=blk)
        blk = r["blk"]
        kinds += r["kinds"]
        parts.append(r)
    assert 8 not in kinds and 9 not in kinds, kinds
    out = {k: torch.cat([p[k] for p in parts]) for k in ("x_out", "c_out", "dx", "dc")}
    out.update(blk=blk, kinds=kinds)
    return out


def _f64(t):
    return t.detach().double().cpu().numpy()


def _maxabs_err(out, ref):
    assert out.shape == ref.shape, (out.shape, ref.shape)
    assert np.isfinite(out).all()
    return float(np.abs(out - ref).max() / max(np.abs(ref).max(), 1e-30))


# ------------------------------------------------------------------------------------------------
# (1) + (2): production-shaped block against the oracle, with the proof that the case reached its leaf
CASES = [("S", 384, 12, 14, 3), ("S", 192, 6, 14, 39), ("D", 192, 6, 28, 11), ("S", 384, 12, 14, 39), ("S", 384, 12, 14, 78), ("S", 384, 12, 14, 154)]


def _expect_kinds(case, kinds):
    kind, C, h, Hs, B = case
    rows = B * (Hs * Hs + MT)
    assert 5 in kinds, kinds                                   # a trainable block: the weight-gradient GEMMs ran
    if rows < 8192:
        assert 8 not in kinds and 9 not in kinds, kinds
    elif C == 192 or rows < 16384 or rows > 32768:
        assert 8 in kinds and 9 not in kinds, kinds
    else:
        assert 8 in kinds and 9 in kinds, kinds


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}{c[1]}-B{c[4]}")
def test_production_block_vs_oracle(cfg, case):
    """Outputs, input gradients and every parameter gradient of the production run (FlatAdamW attached, shipped switches) against the float64 oracle at the block
    budget (2e-2 / 3e-2 of max-abs), and against 1.5 x the error of the yardstick run (see the module docstring) on the same inputs; both sides' errors are
    printed per tensor.  The launch kinds prove the leaf: neither 8 nor 9 at B = 3; 8 without 9 for both C = 192 cases and S / 384 at B = 39; 8 and 9 at B = 78 and
    B = 154.

    Measured on an MI355X (all six cases): the yardstick is inside the budget on every tensor -- outputs <= 5.3e-3, dx / dc <= 7.4e-3, single parameter gradients
    <= 8.9e-3 (norm1.weight at B = 78; production 7.1e-3 there), all parameter gradients in relative L2 4.1e-3 .. 4.5e-3 -- so no tensor takes the 1.5 x yardstick
    bound in place of the budget.  Below the whole-width window the two sides print the same error on every tensor (the register-stationary GEMM and the forward-form
    dX on a transposed copy sum in the tile kernel's order); inside it (B = 78, 154) production / yardstick is 1.00 on the outputs and the L2 figure, 0.96 .. 1.03 on
    dx / dc and 0.74 .. 1.22 on single parameter gradients."""
    kind, C, h, Hs, B = case
    tag = f"{kind} C={C} B={B}"
    prod = _run(case, True)
    _report("train", case, prod["kinds"])
    _expect_kinds(case, prod["kinds"])
    yard = _yardstick(case, cfg)
    ref = _oracle(case)
    failures = []

    def check(what, e_p, e_y, tol, ratio):
        bound = tol if e_y <= tol else MARGIN * e_y          # a tensor on which the yardstick itself is over the budget is bound by the yardstick
        print(f"{tag} {what}: production {e_p:.3e}, yardstick {e_y:.3e} (ratio {e_p / max(e_y, 1e-30):.2f}; bound {bound:.1e})")
        if e_p > bound:
            failures.append(f"{what}: production error {e_p:.3e} > {bound:.3e}")
        if ratio and e_p > MARGIN * e_y:
            failures.append(f"{what}: production error {e_p:.3e} > {MARGIN} x yardstick {e_y:.3e}")

    for k, tol in (("x_out", OUT_TOL), ("c_out", OUT_TOL), ("dx", GRAD_TOL), ("dc", GRAD_TOL)):
        check(k, _maxabs_err(_f64(prod[k]), ref[k]), _maxabs_err(_f64(yard[k]), ref[k]), tol, True)
    gp, gy = dict(prod["blk"].named_parameters()), dict(yard["blk"].named_parameters())
    cat = {"p": [], "y": [], "r": []}
    assert set(ref["grads"]) == set(gp) == set(gy)
    for n, r in ref["grads"].items():
        if np.abs(r).max() == 0:
            continue
        p, y = _f64(gp[n].grad), _f64(gy[n].grad)
        check("grad " + n, _maxabs_err(p, r), _maxabs_err(y, r), GRAD_TOL, False)
        cat["p"].append((p - r).ravel()); cat["y"].append((y - r).ravel()); cat["r"].append(r.ravel())
    nr = np.linalg.norm(np.concatenate(cat["r"]))
    check("parameter gradients, relative L2", float(np.linalg.norm(np.concatenate(cat["p"])) / nr), float(np.linalg.norm(np.concatenate(cat["y"])) / nr), GRAD_TOL, True)
    assert not failures, f"{tag}: " + "; ".join(failures)


@pytest.mark.parametrize("B", [77, 155])
def test_gates_flip_outside_the_window(B):
    """S / 384 one image below (16324 rows) and one above (32860 rows) the whole-width window: the register-stationary GEMM still runs, nothing of kind 9 does."""
    case = ("S", 384, 12, 14, B)
    r = _run(case, True)
    _report("train", case, r["kinds"])
    _expect_kinds(case, r["kinds"])
    assert all(torch.isfinite(r[k].float()).all() for k in ("x_out", "c_out", "dx", "dc"))


def test_dx_ln_bwd_needs_the_transposed_copies():
    """S / 384 at B = 78 without FlatAdamW: the forward-side kind-9 launches still occur (proj + residual + norm2, fc2), the two lmv_linear_dx_ln_bwd launches
    (dX of fc1 + norm2 backward, dX of qkv + norm1 backward) do not -- they need the transposed copies."""
    case = ("S", 384, 12, 14, 78)
    plain = _run(case, False)
    flat = _run(case, True)
    _report("train-no-FlatAdamW", case, plain["kinds"])
    n_plain, n_flat = plain["kinds"].count(9), flat["kinds"].count(9)
    assert 8 in plain["kinds"] and n_plain >= 2, plain["kinds"]
    assert n_flat - n_plain >= 2, (n_plain, n_flat)
    # the forward pass reads the same bf16 weights with and without the optimizer's copies
    assert torch.equal(plain["x_out"], flat["x_out"]) and torch.equal(plain["c_out"], flat["c_out"])


# ------------------------------------------------------------------------------------------------
# (3) inference at the same gates
@pytest.mark.parametrize("B", [78, 154, 155])
def test_fused_inference_at_the_gates(monkeypatch, B):
    """The fused inference schedule (no_grad, LayerNorm folded into qkv, mlp_split384) on the same blocks and inputs, no optimizer: inside the window proj + residual +
    norm2 is one launch and fc2 runs on the whole-width kernel (kind 9); at B = 155 the split MLP runs without either.  Against the oracle forward at 2e-2 of max-abs,
    and bit for bit equal to a second run."""
    from lemevit_amd.blocks import PARAM_NAMES
    M = Mod()
    monkeypatch.setattr(M, "_FUSED", True)
    case = ("S", 384, 12, 14, B)
    kind, C, h, Hs, _ = case
    inp = _inputs(case)
    blk = load(_block(kind, C, h), "blk.", SEED)
    allp = dict(blk.named_parameters())
    params = {n: allp[n] for n in PARAM_NAMES[kind]}
    masks = tuple(m.to(DEV) for m in inp["masks"])
    x, c = inp["x"].to(DEV), inp["c"].to(DEV)
    outs = []
    with torch.no_grad():
        for _ in range(2):
            with _Kinds() as k:
                xo, co = M.run_block(kind, x, c, Hs, Hs, params, masks)
            outs.append((xo.clone(), co.clone(), k.kinds))
    _report("infer", case, outs[0][2])
    assert 8 in outs[0][2] and (9 in outs[0][2]) == (B <= 154), outs[0][2]
    assert outs[0][2] == outs[1][2]
    ref = _oracle(case, grad=False)
    close(outs[0][0], ref["x_out"], OUT_TOL, f"fused inference B={B} x_out"); close(outs[0][1], ref["c_out"], OUT_TOL, f"fused inference B={B} c_out")
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
