"""Attention maps, the parts that need no GPU: the lmv_attn_probs entry point is declared / exported / bound and refuses bad arguments before any
launch, the committed fixtures of the reference's probabilities agree with the float64 oracle, and the host logic of LeMeViT.attention_maps
(block names, the byte bound, query rows, the attn_viz hook points) works on a CPU model."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from detfill import det_tensor, fill_state_dict
from oracle import lemevit_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = {"C": ["meta_from_image"], "D": ["image_from_meta", "meta_from_image"], "D2": ["image_from_meta", "meta_from_image"],
          "S": ["image_self", "meta_self"], "Sx": ["image_self"]}


def call_names(cfg, dense=False):
    """[(block name, field)] of the oracle's sdpa calls in forward order."""
    out = []
    for i, (n, t) in enumerate(zip(cfg["depth"], cfg["attn_type"])):
        kind = "Sx" if (dense and t == "S") else t
        for j in range(n):
            out += [(f"stages.{i}.{j}", f) for f in FIELDS[kind]]
    return out


def recording_sdpa(log):
    """O.sdpa's three lines, keeping softmax(...)."""
    def sdpa(q, k, v, scale=None):
        d = q.shape[-1]
        s = scale if scale is not None else d ** (-0.5)
        attn = (q @ k.transpose(-1, -2)) * s
        attn = attn.softmax(dim=-1)
        log.append(attn.detach())
        return attn @ v
    return sdpa


def oracle_maps(monkeypatch, forward, sd, cfg, img):
    """(outputs, [P per sdpa call]) of the float64 oracle."""
    log = []
    monkeypatch.setattr(O, "sdpa", recording_sdpa(log))
    sd64 = {k: (v.double() if v.dtype.is_floating_point else v) for k, v in sd.items()}
    with torch.no_grad():
        out = forward(sd64, cfg, img.double())
    monkeypatch.undo()
    return out, log


# ------------------------------------------------------------------------------------------------
# 1. the entry point
def test_attn_probs_is_declared_exported_and_bound():
    from lemevit_amd import _lib, ops
    src = open(os.path.join(ROOT, "include", "lemevit_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint\s+lmv_attn_probs\s*\(\s*const\s+lmv_attn_desc\s*\*", src), "not declared in include/lemevit_hip.h"
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "lmv_attn_probs"), "not exported by the library"
    assert "lmv_attn_probs" in _lib.SIGNATURES
    fn = _lib.lib.lmv_attn_probs
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 5
    assert callable(ops.attn_probs)
    assert _lib.ABI_VERSION == 14 and _lib.lib.lmv_abi_version() == 14          # a pure addition
    assert "attnmap.hip" in open(os.path.join(ROOT, "lemevit_amd", "csrc", "Makefile")).read()
    with pytest.raises(RuntimeError, match="GPU"):
        ops.attn_probs((torch.zeros(1, 16, 64), 0), (torch.zeros(1, 16, 64), 0), torch.zeros(1, 2, 16), 64, 0.2)


# ------------------------------------------------------------------------------------------------
# 2. argument refusal before any launch
def _desc(**kw):
    from lemevit_amd._lib import AttnDesc
    d = AttnDesc()
    d.q, d.k, d.lse = 0x10000, 0x20000, 0x30000          # never dereferenced: every case below is refused on the host
    d.q_bs, d.q_rs, d.k_bs, d.k_rs = 16 * 96, 96, 3136 * 192, 192
    d.B, d.H, d.Lq, d.Lk, d.scale = 2, 3, 16, 3136, 0.1
    for k, v in kw.items():
        setattr(d, k, v)
    return d


SHAPE_CASES = [("null q", dict(q=None)), ("null k", dict(k=None)), ("null lse", dict(lse=None)), ("misaligned q", dict(q=0x10008)), ("misaligned k", dict(k=0x20004)),
               ("q_rs % 8", dict(q_rs=100)), ("q_bs % 8", dict(q_bs=16 * 96 + 4)), ("k_rs % 8", dict(k_rs=190)), ("k_bs % 8", dict(k_bs=3136 * 192 + 1)),
               ("B = 0", dict(B=0)), ("H < 0", dict(H=-1)), ("Lq = 0", dict(Lq=0)), ("Lk = 0", dict(Lk=0)), ("scale = 0", dict(scale=0.0)),
               ("scale < 0", dict(scale=-0.5)), ("scale NaN", dict(scale=float("nan"))), ("plane 2^31", dict(Lq=1 << 16, Lk=1 << 15))]


def test_attn_probs_refuses_bad_arguments_without_a_launch():
    from lemevit_amd._lib import lib, LMV_BF16, LMV_F32
    P = 0x40000

    def call(d, p=P, mean=0, dtype=LMV_BF16):
        rc = lib.lmv_attn_probs(None if d is None else ctypes.byref(d), p, mean, dtype, None)
        return rc, lib.lmv_last_error()

    for dtype in (LMV_F32, LMV_BF16):
        for what, kw in SHAPE_CASES:
            for mean in (0, 1):
                rc, msg = call(_desc(**kw), mean=mean, dtype=dtype)
                assert rc == -1 and b"attn_probs" in msg, (what, rc, msg)
    for what, d, p in [("null descriptor", None, P), ("null p", _desc(), None), ("misaligned p", _desc(), P + 4)]:
        rc, msg = call(d, p)
        assert rc == -1 and b"attn_probs" in msg, (what, rc, msg)
    assert (1 << 16) * ((1 << 15) - 1) < 1 << 31          # ... and the plane just below the bound is a dtype error only because of its dtype
    for dtype in (2, -1, 7):
        rc, msg = call(_desc(), dtype=dtype)
        assert rc == -2 and b"attn_probs" in msg, (dtype, rc, msg)
        rc, msg = call(_desc(Lq=1 << 16, Lk=(1 << 15) - 1), dtype=dtype)
        assert rc == -2 and b"attn_probs" in msg, (dtype, rc, msg)


# ------------------------------------------------------------------------------------------------
# 3. the oracle against the reference's fixtures
def _check_fixture(meta, g, log, names):
    assert [c[:2] for c in meta["calls"]] == [list(n) for n in names] and len(log) == len(names)
    worst = 0.0
    for n, ((blk, field, Lq, Lk), p) in enumerate(zip(meta["calls"], log)):
        assert tuple(p.shape[-2:]) == (Lq, Lk)
        pairs = [(p.mean(1), g[f"mean.{n}"])] + ([(p, g[f"heads.{n}"])] if f"heads.{n}" in g else [])
        assert (f"heads.{n}" in g) == (blk in meta["per_head_blocks"])
        for got, want in pairs:
            want = torch.from_numpy(want).double()
            assert got.shape == want.shape, (n, blk, field)
            err = float((got - want).abs().max() / want.abs().max())
            worst = max(worst, err)
            assert err <= 1e-5, (n, blk, field, err)
            assert float((want - 1.0 / Lk).abs().max()) >= 1e-3 * float(want.abs().max()), "a fixture map must stand clear of the uniform map"
    print(f"oracle vs reference maps: worst {worst:.2e} of max-abs over {len(log)} calls")
    assert len(g["bf16_dev"]) == len(log) and float(g["bf16_dev"].max()) < 0.2
    return worst


def test_oracle_reproduces_the_reference_maps(golden, monkeypatch):
    meta, g = golden("attnmap_tiny_96")
    cfg = O.VARIANTS[meta["variant"]]
    sd = fill_state_dict(O.state_dict_spec(cfg, meta["num_classes"]), meta["seed"])
    img = det_tensor((meta["B"], 3, meta["res"], meta["res"]), meta["img"], meta["img_seed"])
    logits, log = oracle_maps(monkeypatch, O.lemevit_forward, sd, cfg, img)
    assert len(log) == 29
    _check_fixture(meta, g, log, call_names(cfg))
    assert float((logits - torch.from_numpy(g["out0"]).double()).abs().max()) <= 1e-5 * float(np.abs(g["out0"]).max())


def test_oracle_reproduces_the_reference_maps_dense(golden, monkeypatch):
    meta, g = golden("attnmap_dense_tiny_160x96")
    cfg = meta["cfg"]
    sd = fill_state_dict(O.state_dict_spec(cfg, 0), meta["seed"])
    img = det_tensor((meta["B"], 3, meta["H"], meta["W"]), meta["img"], meta["img_seed"])
    outs, log = oracle_maps(monkeypatch, O.lemevit_dense_forward, sd, cfg, img)
    names = call_names(cfg, dense=True)
    assert len(outs) == 4 and not any(f == "meta_self" for _, f in names)
    _check_fixture(meta, g, log, names)


# ------------------------------------------------------------------------------------------------
# 4. host logic of attention_maps
def test_attention_maps_host_logic():
    import lemevit_amd as L
    import lemevit_amd.model as M
    m = L.create_model("lemevit_tiny", num_classes=10)
    img = torch.zeros(2, 3, 96, 96)
    with pytest.raises(ValueError, match="stages.9.0"):
        m.attention_maps(img, blocks=["stages.1.0", "stages.9.0"])
    with pytest.raises(ValueError, match="heads"):
        m.attention_maps(img, heads="max")
    with pytest.raises(ValueError, match="image_queries"):
        m.attention_maps(img, image_queries=[(0.5, 1.0)])
    # the byte bound is checked on shapes alone, before the GPU is touched (a CPU model and a CPU image get this far and no further)
    big = torch.zeros(1, 3, 800, 1344)
    with pytest.raises(ValueError, match=r"423366144 bytes.*blocks=.*image_queries="):
        m.attention_maps(big, blocks=["stages.3.0"], heads="all", image_queries="all", max_bytes=1 << 28)
    with pytest.raises(ValueError, match="max_bytes = 1073741824"):          # the default bound: 1 GiB; three such blocks pass it
        m.attention_maps(big, blocks=["stages.3.0", "stages.3.1", "stages.3.2"], heads="all", image_queries="all")
    plan, total = m._map_plan((1, 3, 800, 1344), ["stages.3.0"], "all", "all")
    assert total == 4 * 6 * (4200 * 4200 + 16 * 16) and plan[0][2] == (50, 84)
    with pytest.raises(RuntimeError, match="MI355X|GPU"):          # under the bound the call goes on to the device, which a CPU image does not have
        m.attention_maps(img)
    assert m.training, "the module keeps its mode"
    # every block, head-mean, no image queries at 96 x 96: 15 blocks, the D / C maps and the meta self-attention only
    plan, total = m._map_plan((2, 3, 96, 96))
    assert [p[0] for p in plan] == [f"stages.{i}.{j}" for i, n in enumerate([1, 2, 2, 8, 2]) for j in range(n)]
    assert [p[2] for p in plan] == [(24, 24)] * 3 + [(12, 12)] * 2 + [(6, 6)] * 8 + [(3, 3)] * 2
    assert dict(plan[1][3]) == {"image_from_meta": (2, 24, 24, 16), "meta_from_image": (2, 16, 24, 24)} and dict(plan[5][3]) == {"meta_self": (2, 16, 16)}
    assert total == 4 * 2 * (16 * 576 * 5 + 16 * 144 * 4 + 256 * 10)
    _, with_rows = m._map_plan((2, 3, 96, 96), image_queries=[(0.5, 0.5), (0.0, 0.99)])
    assert with_rows - total == 4 * 2 * 2 * (36 * 8 + 9 * 2)
    assert dict(m._map_plan((2, 3, 96, 96), ["stages.3.0"], "all", "all")[0][0][3]) == {"image_self": (2, 6, 36, 6, 6), "meta_self": (2, 6, 16, 16)}
    # odd sizes follow the stride-2 convolutions: 3 x 3, padding 1 -> (n + 1) // 2
    assert [p[2] for p in m._map_plan((1, 3, 97, 131), ["stages.0.0", "stages.2.0", "stages.4.1"])[0]] == [(25, 33), (13, 17), (4, 5)]
    # (fy, fx) -> row
    assert M.map_query_rows([(0.5, 0.5), (0.0, 0.99)], 6, 6) == [21, 5] and M.map_query_rows([(0.5, 0.5), (0.0, 0.99)], 3, 3) == [4, 2]
    assert M.map_query_rows([(0.999, 0.999)], 50, 84) == [4199] and M.map_query_rows(None, 6, 6) == [] and M.map_query_rows("all", 6, 6) is None
    with pytest.raises(ValueError):
        M.map_query_rows("some", 6, 6)
    with pytest.raises(ValueError):
        M.map_query_rows([(-0.1, 0.5)], 6, 6)


def test_attn_viz_hook_points_leave_the_state_dict_alone():
    import lemevit_amd as L
    import lemevit_amd.model as M
    for cls in (M.StandardAttention, M.DualCrossAttention, M.DualCrossAttention_v2, M.CrossAttention):
        a = cls(dim=64, num_heads=2)
        assert isinstance(a.attn_viz, torch.nn.Identity) and not any(k.startswith("attn_viz") for k in a.state_dict())
    for variant in ("lemevit_tiny", "lemevit_tiny_v2"):
        m = L.create_model(variant, num_classes=10)
        spec = O.state_dict_spec(O.VARIANTS[variant], 10)
        assert list(m.state_dict().keys()) == list(spec.keys())
        assert all(isinstance(blk.attn.attn_viz, torch.nn.Identity) for st in m.stages for blk in st)
    bb = M.LeMeViTBackbone(depth=[1, 1, 1, 1, 1], embed_dim=[64, 64, 128, 192, 320], head_dim=32, attn_type=["C", "D", "D", "S", "S"], queries_len=16)
    plan, _ = bb._map_plan((1, 3, 64, 64), image_queries=[(0.5, 0.5)])
    assert [dict(p[3]).keys() for p in plan][3:] == [{"image_self"}, {"image_self"}], "the dense backbone's S blocks have no meta_self"
    assert [len(p[3]) for p in bb._map_plan((1, 3, 64, 64))[0]] == [1, 2, 2, 0, 0]


# ------------------------------------------------------------------------------------------------
# the wiring the stand-alone attention modules and the map recorder share with the block schedules (lemevit_amd/blocks.py)
def test_attention_halves_share_parameter_names_and_saved_fields(monkeypatch):
    """The modules hand their (weight, bias) pairs to the attention halves by the block's parameter names, and LeMeViT.attention_maps reads the saved set by
    field name: a module whose Linears are declared in another order than blocks.PARAM_NAMES, or a kind whose saved set has other fields, would feed a kernel
    the wrong operand.  The launches are stubbed (no GPU): only the host wiring runs, on a module's data (no norm1, no residual)."""
    from lemevit_amd import blocks, model, ops
    classes = {"S": model.StandardAttention, "D": model.DualCrossAttention, "D2": model.DualCrossAttention_v2, "C": model.CrossAttention}
    monkeypatch.setattr(ops, "linear_fwd", lambda probs, N, K, act=0: None)
    monkeypatch.setattr(ops, "attn_fwd", lambda q, k, v, C_, scale, want_lse=False, stream=None: (q[0].new_empty(q[0].shape[:-1] + (C_,)), q[0].new_empty(1)))
    C, x, c = 64, torch.zeros(2, 9, 64), torch.zeros(2, 4, 64)
    for kind, cls in classes.items():
        m = cls(dim=C, num_heads=C // 32)
        names = [n for n in blocks.PARAM_NAMES[kind] if n.startswith("attn.")]
        assert names == ["attn." + n for n, _ in m.named_parameters()], kind
        assert names == ["attn." + n for n in m.state_dict()], kind
        P = {n: p.detach() for n, p in zip(names, m.parameters())}
        ts = [x] if kind == "S" else [x, c]
        outs, saved = blocks.ATTN_FWD[kind](P, ts, None, True)
        assert type(saved) is blocks.AttnSaved and saved._fields == ("ts", "st", "xn", "proj", "ao", "lse"), kind
        assert all(isinstance(getattr(saved, f), list) for f in saved._fields), kind
        assert len(saved.ts) == len(saved.st) == len(saved.xn) == len(saved.proj) == len(ts) and len(saved.ao) == len(saved.lse) == len(outs), kind
        assert all(a is b for a, b in zip(saved.xn, ts)), "without norm1 the in-projections read the streams themselves"
    assert set(blocks.ATTN_FWD) == set(blocks.ATTN_BWD) == set(blocks.PARAM_NAMES)
