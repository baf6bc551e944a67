"""Frozen parameters, the parts that need no GPU: the additions to the C ABI are declared / exported / bound (ABI still 14), LMV_BLOCK_DATA_ONLY shrinks the
saved set by exactly the n1 / n2 / h tensors of csrc/block.hip::layout_fwd, lmv_block_bwd accepts NULL gradient pointers with the flag (and only with it), the
fused dX kernel of the MLP half compiles for gfx950 without scratch, and -- on the oracle -- freezing stages 0 and 1 changes no gradient that remains
(the claim the GPU tests of tests/test_frozen_params_gpu.py build on, pinned to the reference's train_tiny_96 fixture)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from detfill import det_tensor, fill_state_dict
from oracle import lemevit_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lemevit_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
NEW = ["lmv_block_fwd_scratch_bytes", "lmv_block_fwd_range_scratch", "lmv_mlp_dx_fused", "lmv_mlp_dx_fused_supported", "lmv_debug_wgrad_launches"]
DATA_ONLY = 4


# ------------------------------------------------------------------------------------------------
# (a) exports
def test_new_symbols_declared_exported_bound():
    from lemevit_amd import _lib
    with open(os.path.join(ROOT, "include", "lemevit_hip.h")) as f:
        src = f.read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, src), n + ": not declared in include/lemevit_hip.h"
        assert hasattr(raw, n), n + ": not exported by the library"
        assert n in _lib.SIGNATURES and getattr(_lib.lib, n).argtypes is not None, n + ": not bound"
    assert _lib.ABI_VERSION == 14 and _lib.lib.lmv_abi_version() == 14 and re.search(r"#define\s+LMV_ABI_VERSION\s+14\b", src)
    assert re.search(r"\bLMV_BLOCK_DATA_ONLY\s*=\s*4\b", src) and _lib.BLOCK_DATA_ONLY == DATA_ONLY
    from lemevit_amd import ops
    assert callable(ops.mlp_dx_fused) and callable(ops.mlp_dx_fused_supported) and isinstance(ops.wgrad_launches(), int)
    assert _lib.config_get("mlp_dx_fused") in (0, 1, 2)
    _lib.config_set("mlp_dx_fused", 2)
    try:
        assert _lib.config_get("mlp_dx_fused") == 2
    finally:
        _lib.config_set("mlp_dx_fused", 1)
    for C, hid, dt, ok in [(96, 384, 1, True), (192, 768, 1, True), (384, 1536, 1, True), (64, 256, 1, True), (384, 1536, 0, False), (512, 2048, 1, False), (96, 200, 1, False)]:
        assert bool(_lib.lib.lmv_mlp_dx_fused_supported(C, hid, dt)) == ok == bool(_lib.lib.lmv_mlp_fused_supported(C, hid, dt)), (C, hid, dt)


# ------------------------------------------------------------------------------------------------
# (b) arena size
KINDS = {"S": 0, "D": 1, "C": 2}
SHAPES = [("S", 384, 128, 14, 14), ("D", 192, 128, 28, 28), ("C", 96, 128, 56, 56)]          # N = 196, 784, 3136


def _desc(kind, C, B, H, W, dtype, flags=0, params=True):
    from lemevit_amd._lib import BlockDesc
    d = BlockDesc()
    d.kind, d.dtype, d.B, d.H, d.W, d.M, d.C, d.hidden, d.eps, d.flags = KINDS[kind], dtype, B, H, W, 16, C, 4 * C, 1e-6, flags
    if params:
        p = 1 << 20          # a non-null, aligned address: no call below reaches a launch
        for f in ("pos_w", "pos_b", "n1_w", "n1_b", "n2_w", "n2_b", "fc1_w", "fc1_b", "fc2_w", "fc2_b"):
            setattr(d, f, p)
        for i in range(4):
            d.attn_w[i] = p; d.attn_b[i] = p
    return d


@pytest.mark.parametrize("dtype", [0, 1], ids=["fp32", "bf16"])
@pytest.mark.parametrize("kind,C,B,H,W", SHAPES)
def test_arena_shrinks_by_n1_n2_h(kind, C, B, H, W, dtype):
    from lemevit_amd._lib import lib
    es, M, Hd = (2 if dtype == 1 else 4), 16, 4 * C
    rows = [B * H * W, B * M]
    full = lib.lmv_block_arena_bytes(ctypes.byref(_desc(kind, C, B, H, W, dtype)))
    part = lib.lmv_block_arena_bytes(ctypes.byref(_desc(kind, C, B, H, W, dtype, DATA_ONLY)))
    tr = lib.lmv_block_fwd_scratch_bytes(ctypes.byref(_desc(kind, C, B, H, W, dtype)))
    assert full > 0 and part > 0 and tr > 0
    # csrc/block.hip::layout_fwd: n1 for both streams; n2 and h for every stream that runs the MLP half (a "C" block: the meta tokens only)
    sizes = []
    for s in range(2):
        sizes.append(rows[s] * C * es)
        if not (kind == "C" and s == 0):
            sizes += [rows[s] * C * es, rows[s] * Hd * es]
    want = sum(sizes)
    print(f"{kind} C={C} dtype={dtype}: full {full} data-only {part} ({part / full:.3f}), difference {full - part} vs n1 + n2 + h = {want}; transient {tr}")
    assert abs((full - part) - want) <= 256 * len(sizes), (full, part, want)
    assert tr >= full - part
    if kind == "S":
        assert part < 0.65 * full, "an S block keeps 10 C of 16 C per row"
    # the backward scratch does not depend on the flag
    assert lib.lmv_block_bwd_scratch_bytes(ctypes.byref(_desc(kind, C, B, H, W, dtype))) == lib.lmv_block_bwd_scratch_bytes(ctypes.byref(_desc(kind, C, B, H, W, dtype, DATA_ONLY)))


@pytest.mark.parametrize("kind", ["S", "D", "C"])
def test_block_bwd_null_gradient_pointers_need_the_flag(kind):
    from lemevit_amd._lib import lib
    p = 1 << 20

    def bwd(d, c=p, x=p):     # c = NULL stops every call at the tensor check that FOLLOWS the parameter / gradient pointer check: nothing is launched
        return lib.lmv_block_bwd(ctypes.byref(d), x, c, p, 1 << 30, p, p, p, p, p, 1 << 30, None, None)

    assert bwd(_desc(kind, 96, 2, 8, 8, 1), c=None) == -1 and b"null gradient pointer" in lib.lmv_last_error()
    assert bwd(_desc(kind, 96, 2, 8, 8, 1, DATA_ONLY), c=None) == -1 and b"null / misaligned tensor" in lib.lmv_last_error(), lib.lmv_last_error()
    # x feeds the position convolution's weight gradient alone: with the flag it may be NULL (the call gets past the tensor check and stops at the arena size)
    d = _desc(kind, 96, 2, 8, 8, 1, DATA_ONLY)
    assert lib.lmv_block_bwd(ctypes.byref(d), None, p, p, 256, p, p, p, p, p, 1 << 30, None, None) != 0 and b"block_bwd: arena" in lib.lmv_last_error(), lib.lmv_last_error()
    assert bwd(_desc(kind, 96, 2, 8, 8, 1, DATA_ONLY, params=False)) == -1 and b"null parameter pointer" in lib.lmv_last_error()
    # the forward refuses the flag without its transient buffer, and a transient buffer that is too small
    d = _desc(kind, 96, 2, 8, 8, 1, DATA_ONLY)
    assert lib.lmv_block_fwd(ctypes.byref(d), p, p, p, p, p, 1 << 30, 1, None) == -1 and b"transient" in lib.lmv_last_error()
    assert lib.lmv_block_fwd_range(ctypes.byref(d), p, p, p, p, p, 1 << 30, 1, 0, 1, None) == -1 and b"transient" in lib.lmv_last_error()
    assert lib.lmv_block_fwd_range_scratch(ctypes.byref(d), p, p, p, p, p, 1 << 30, 1, 0, 1, p, 256, None) == -3 and b"transient" in lib.lmv_last_error()
    assert lib.lmv_block_fwd_range_scratch(ctypes.byref(d), p, p, p, p, p, 1 << 30, 1, 0, 3, p, 1 << 30, None) == -1 and b"outside the batch" in lib.lmv_last_error()


def test_dx_only_layernorm_and_fused_dx_refuse_bad_arguments():
    from lemevit_amd import _lib
    lib, p = _lib.lib, 1 << 20
    seg = (_lib.LnSegment * 1)()
    seg[0].x, seg[0].dy, seg[0].stats, seg[0].dx, seg[0].rows = p, p, p, p, 4
    rows = ctypes.c_int(0)
    # partial rows without a workspace is still an error (dx-only mode is: neither); C = 20 stops the dx-only form before any launch
    assert lib.lmv_layernorm_bwd_partial(seg, 1, p, 96, None, 0, ctypes.byref(rows), 1, None) == -3
    assert lib.lmv_layernorm_bwd_partial(seg, 1, p, 20, None, 0, None, 1, None) == -1 and b"multiple of 8" in lib.lmv_last_error()
    assert lib.lmv_layernorm_bwd_partial(None, 1, p, 96, None, 0, None, 1, None) == -1
    q = (_lib.MlpDxProblem * 1)()
    q[0].g, q[0].u, q[0].dn2, q[0].rows = p, p, p, 100
    for kw in [dict(C=100), dict(hid=200), dict(w2=None), dict(w1=None), dict(n=0), dict(n=3)]:
        a = dict(C=96, hid=384, w2=p, w1=p, n=1, dt=1); a.update(kw)
        assert lib.lmv_mlp_dx_fused(q, a["n"], a["w2"], a["w1"], a["C"], a["hid"], a["dt"], None) == -1, kw
    assert lib.lmv_mlp_dx_fused(q, 1, p, p, 96, 384, 0, None) == -2
    q[0].u = None
    assert lib.lmv_mlp_dx_fused(q, 1, p, p, 96, 384, 1, None) == -1 and b"mlp_dx_fused" in lib.lmv_last_error()


# ------------------------------------------------------------------------------------------------
# (c) the fused dX kernel's resources
@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="no hipcc in this environment")
def test_fused_dx_kernel_resources(tmp_path):
    """Every instance of the fused dX kernel (mlp_fused_kernel<C, TM, DX = true>, csrc/fused.hip) on gfx950: no scratch (a spill in the chunk loop would
    put private-memory traffic under every MFMA step) and at most 160 KB of LDS.  The kernel's LDS is dynamic -- MlpCfg::LDS, bounded by a static_assert
    against the 160 KB / 80 KB budget, so a layout that outgrows it fails this compile -- and the remark reports the static part."""
    cmd = [HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-munsafe-fp-atomics", "--cuda-device-only", "-c", os.path.join(CSRC, "fused.hip"), "-o",
           str(tmp_path / "fused.o"), "-Rpass-analysis=kernel-resource-usage"]
    r = subprocess.run(cmd, check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    found = {}
    for blk in re.split(r"remark: Function Name: ", r.stderr)[1:]:
        name = blk.split()[0]
        m = re.search(r"mlp_fused_kernelILi(\d+)ELi(\d+)ELb1E", name)
        if not m:
            continue
        val = lambda key: int(re.search(re.escape(key) + r": (\d+)", blk).group(1))
        found[(int(m.group(1)), int(m.group(2)))] = (val("ScratchSize [bytes/lane]"), val("LDS Size [bytes/block]"), val("VGPRs Spill"), val("VGPRs"), val("AGPRs"))
    print(found)
    assert {(C, 128) for C in (64, 96, 128, 192, 256, 320, 384)} <= set(found) and {(C, 64) for C in (64, 96, 128, 192)} <= set(found), sorted(found)
    for key, (scratch, lds, spill, vgpr, agpr) in found.items():
        assert scratch == 0 and spill == 0, f"lmv_mlp_dx_fused instance {key}: {scratch} bytes of scratch per lane, {spill} spilled VGPRs"
        assert lds <= 160 * 1024, (key, lds)
        assert vgpr + agpr <= 512, (key, vgpr, agpr)


# ------------------------------------------------------------------------------------------------
# (d) freezing changes no gradient that remains
def test_oracle_frozen_stages_leave_the_remaining_gradients(golden):
    """train_tiny_96 with the parameters of stages 0 and 1 frozen: loss, logits and every remaining parameter's gradient are the fixture's, at
    tests/test_oracle_golden.py::test_train_step's tolerances; the frozen parameters get none."""
    meta, g = golden("train_tiny_96")
    cfg = O.VARIANTS[meta["variant"]]
    sd = fill_state_dict(O.state_dict_spec(cfg, meta["num_classes"]), meta["seed"])
    frozen = ("stages.0.", "stages.1.")
    for k, v in sd.items():
        if v.dtype.is_floating_point and not k.endswith(("running_mean", "running_var")) and not k.startswith(frozen):
            v.requires_grad_(True)
    img = det_tensor((meta["B"], 3, meta["res"], meta["res"]), "train_tiny_96.img", 5)
    logits = O.lemevit_forward(sd, cfg, img, train=True, new_stats={})
    loss = torch.nn.functional.cross_entropy(logits, torch.tensor(meta["target"]))
    loss.backward()
    assert abs(loss.item() - float(g["loss"])) < 1e-5
    names = list(meta["param_names"])
    assert any(k.startswith(frozen) for k in names)
    checked = 0
    for i, k in enumerate(names):
        if k.startswith(frozen):
            assert sd[k].grad is None, k
            continue
        gn = float(sd[k].grad.norm()) if sd[k].grad is not None else 0.0
        assert abs(gn - g["grad_norms"][i]) <= 3e-4 * max(1.0, abs(g["grad_norms"][i])), (k, gn, g["grad_norms"][i])
        checked += 1
    assert checked > 50
    full = 0
    for k in g:
        if k.startswith("grad.") and k != "grad_norms" and not k[5:].startswith(frozen):
            a, b = sd[k[5:]].grad.double().numpy(), np.asarray(g[k], dtype=np.float64)
            assert np.abs(a - b).max() <= 1e-4 * max(1.0, np.abs(b).max()), k
            full += 1
    assert full >= 1
