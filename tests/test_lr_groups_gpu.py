"""Per-group and scheduled learning rates on a real MI355X: lmv_adamw_flat_groups bit for bit against the scalar kernels run slice by slice, against
torch.optim.AdamW with parameter groups, the table read at run time, FlatAdamW(layer_decay=...) on a whole model against torch.optim.AdamW with one group per
parameter, and a scheduled rate followed by a captured step (GraphedStep(before_replay=opt.sync_hyper))."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from detfill import det_tensor

DEV = "cuda:0"
UNIT = 8
UNITS = [1, 3, 1537, 2, 515]          # slice lengths in units of 8 elements: 16 464 elements, boundaries off every workgroup multiple
GROUP = [0, 1, 2, 1, 0]               # the groups are not contiguous
TABLE = [(1e-2, 0.05), (3e-3, 0.0), (7e-4, 0.1)]          # (lr, weight_decay) per group; group 1 does not decay
BIG = 2048 * 256 * 4 + 8 * 5          # one element group more than the capped grid covers in a sweep: the grid-stride loop runs a second time
B1, B2 = 0.9, 0.999


def ops():
    from lemevit_amd import ops as _ops
    return _ops


def _slices(units):
    out, off = [], 0
    for u, gi in zip(units, GROUP):
        out.append((off * UNIT, (off + u) * UNIT, gi))
        off += u
    return out


def _buffers(n, zero_moments=False):
    p = det_tensor((n,), "lrg.p", 7).to(DEV); g = det_tensor((n,), "lrg.g", 7, 0.1).to(DEV)
    m = torch.zeros_like(p) if zero_moments else det_tensor((n,), "lrg.m", 7, 0.01).to(DEV)
    v = torch.zeros_like(p) if zero_moments else det_tensor((n,), "lrg.v", 7, 0.01).abs().to(DEV)
    return [p, g, m, v, p.to(torch.bfloat16)]


def _index(units):
    return torch.cat([torch.full((u,), gi, dtype=torch.uint8) for u, gi in zip(units, GROUP)]).to(DEV)


def _stat(coef):
    st = torch.zeros(ops().GRAD_STAT_FLOATS, device=DEV)
    st[1], st[2] = coef, 1.0 / coef
    return st


def _per_slice(bufs, units, table, step, mask, eps=1e-8, **kw):
    """the reference: the scalar entry point on every slice's sub-range with its group's scalars"""
    p, g, m, v, sh = bufs
    for s, e, gi in _slices(units):
        lr, wd = table[gi]
        ops().adamw_flat(p[s:e], g[s:e], m[s:e], v[s:e], None if mask is None else mask[s:e], lr, B1, B2, eps, wd, step, shadow=sh[s:e], **kw)


def _grouped(bufs, units, table, step, eps=1e-8, **kw):
    p, g, m, v, sh = bufs
    tb = table if torch.is_tensor(table) else torch.tensor(table, dtype=torch.float32, device=DEV)
    ops().adamw_flat_groups(p, g, m, v, _index(units), tb, B1, B2, eps, step, shadow=sh, **kw)


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


# ---- 1. exact against the existing kernels ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["plain", "stat", "clamp", "stat+clamp"])
@pytest.mark.parametrize("mask", ["ones", "none"])
def test_grouped_equals_scalar_kernels_slice_by_slice(mode, mask):
    """Three steps of ONE grouped launch over five slices of three groups equal, bit for bit in p, m, v and the bf16 copy, three steps of the scalar kernel on
    every slice with its group's (lr, weight_decay): lmv_adamw_flat for the plain step, lmv_adamw_flat_clip with a coefficient (0.37) and / or a clamp (0.05).
    The scalar side runs with the all-ones decay mask FlatAdamW hands it, and without a mask."""
    n = sum(UNITS) * UNIT
    assert n == 16464
    kw = {}
    if "stat" in mode:
        kw["stat"] = _stat(0.37)
    if "clamp" in mode:
        kw["clip_value"] = 0.05
    ref, got = _buffers(n), _buffers(n)
    ones = torch.ones(n, device=DEV) if mask == "ones" else None
    for step in range(1, 4):
        _per_slice(ref, UNITS, TABLE, step, ones, **kw)
        _grouped(got, UNITS, TABLE, step, **kw)
    assert torch.isfinite(got[0]).all() and not torch.equal(got[0], _buffers(n)[0])
    for name, a, b in zip("p g m v shadow".split(), ref, got):
        assert torch.equal(a, b), f"{mode}: {name} differs in {int((a != b).sum())} of {n} elements"
    assert torch.equal(got[4], got[0].to(torch.bfloat16))


def test_grouped_equals_scalar_kernels_with_device_step_count():
    n = sum(UNITS) * UNIT
    ref, got = _buffers(n), _buffers(n)
    step = torch.zeros((), device=DEV, dtype=torch.int32)
    for _ in range(3):
        step += 1
        _per_slice(ref, UNITS, TABLE, 0, None, step_dev=step)
        _grouped(got, UNITS, TABLE, 0, step_dev=step)
    assert _same(ref, got)


def test_grouped_second_sweep_of_the_grid_stride_loop():
    """n = 2048 * 256 * 4 + 40 elements: grid_for caps the grid at 2048 workgroups, so the last ten 16-byte groups are a second trip of the loop."""
    units = [1, 3, 1537, 2, BIG // UNIT - 1543]
    assert sum(units) * UNIT == BIG and BIG // 4 > 2048 * 256
    ref, got = _buffers(BIG), _buffers(BIG)
    for step in range(1, 4):
        _per_slice(ref, units, TABLE, step, None)
        _grouped(got, units, TABLE, step)
    assert _same(ref, got)
    tail = slice(2048 * 256 * 4, BIG)
    assert not torch.equal(got[0][tail], _buffers(BIG)[0][tail]), "the second sweep must have run"


def test_grouped_skipped_step_writes_nothing():
    n = sum(UNITS) * UNIT
    bufs = _buffers(n)
    before = [t.clone() for t in bufs]
    st = torch.zeros(ops().GRAD_STAT_FLOATS, device=DEV)
    st[3] = 1.0                                         # found_inf with coefficient 0: what lmv_grad_norm leaves under LMV_NORM_SKIP_NONFINITE
    _grouped(bufs, UNITS, TABLE, 1, stat=st)
    assert _same(before, bufs)
    st[1] = 1.0                                         # control: the same launch with a coefficient moves everything
    _grouped(bufs, UNITS, TABLE, 1, stat=st)
    assert not any(torch.equal(a, b) for a, b in zip(before[2:], bufs[2:])) and not torch.equal(before[0], bufs[0])


def test_group_byte_out_of_range_reads_the_last_entry():
    """The host never writes one; the kernel clamps it to ngroups - 1 rather than read past the table."""
    n = sum(UNITS) * UNIT
    a, b = _buffers(n), _buffers(n)
    p, g, m, v, sh = a
    idx = _index(UNITS)
    wild = idx.clone()
    wild[idx == 2] = 200
    tb = torch.tensor(TABLE, dtype=torch.float32, device=DEV)
    ops().adamw_flat_groups(p, g, m, v, wild, tb, B1, B2, 1e-8, 1, shadow=sh)
    _grouped(b, UNITS, TABLE, 1)
    assert _same(a, b)


# ---- 2. against torch.optim.AdamW ------------------------------------------------------------------------------------------------------------
def _torch_err(table_for_kernel):
    """max-abs difference, relative to max |p|, between three grouped steps with `table_for_kernel` and torch.optim.AdamW with the three groups of TABLE"""
    n = sum(UNITS) * UNIT
    bufs = _buffers(n, zero_moments=True)
    p, g = bufs[0], bufs[1]
    params = [torch.nn.Parameter(p[s:e].clone()) for s, e, _ in _slices(UNITS)]
    opt = torch.optim.AdamW([dict(params=[q for q, (_, _, gi) in zip(params, _slices(UNITS)) if gi == k], lr=TABLE[k][0], weight_decay=TABLE[k][1])
                             for k in range(3)], betas=(B1, B2), eps=1e-2)
    for step in range(1, 4):
        for q, (s, e, _) in zip(params, _slices(UNITS)):
            q.grad = g[s:e].clone()
        opt.step()
        _grouped(bufs, UNITS, table_for_kernel, step, eps=1e-2)
    ref = torch.cat([q.detach() for q in params])
    assert torch.isfinite(p).all() and torch.equal(bufs[4], p.to(torch.bfloat16))
    return float((p - ref).abs().max()) / float(ref.abs().max())


def test_grouped_against_torch_adamw_param_groups():
    """eps = 1e-2 and the tolerance 1e-5 of max |p| are test_adamw_flat's own budget (tests/test_clip_grad_gpu.py reuses it too).  Control: the same reference
    against a table that holds group 0's rate in every row must miss it."""
    e = _torch_err(TABLE)
    c = _torch_err([(TABLE[0][0], wd) for _, wd in TABLE])
    print(f"grouped vs torch.optim.AdamW with three groups: rel err {e:.3e} (control, group 0's rate everywhere: {c:.3e})")
    assert e <= 1e-5 < c


# ---- 3. the table is read at run time ---------------------------------------------------------------------------------------------------------
def test_table_is_read_by_the_running_kernel():
    """Two launches with identical host arguments (the step count lives on the device too); between them groups[1, 0] is rewritten ON THE DEVICE.  The second result
    is the per-slice reference with the new rate, bit for bit -- and not the one with the old rate."""
    n = sum(UNITS) * UNIT
    got, ref, stale = _buffers(n), _buffers(n), _buffers(n)
    tb = torch.tensor(TABLE, dtype=torch.float32, device=DEV)
    idx = _index(UNITS)
    step = torch.ones((), device=DEV, dtype=torch.int32)
    new_rate = torch.tensor(9e-3, dtype=torch.float32, device=DEV)
    after = [TABLE[0], (float(new_rate), TABLE[1][1]), TABLE[2]]          # the float32 value, as a host float: what the scalar kernel takes as an argument

    def launch():
        p, g, m, v, sh = got
        ops().adamw_flat_groups(p, g, m, v, idx, tb, B1, B2, 1e-8, 0, shadow=sh, step_dev=step)
    launch()
    tb[1, 0].copy_(new_rate)
    step += 1
    launch()
    for bufs, second in ((ref, after), (stale, TABLE)):
        _per_slice(bufs, UNITS, TABLE, 1, None)
        _per_slice(bufs, UNITS, second, 2, None)
    assert _same(ref, got)
    assert not torch.equal(stale[0], got[0])


# ---- 4. whole model -----------------------------------------------------------------------------------------------------------------------------
def _twin(**kw):
    import lemevit_amd
    torch.manual_seed(0)
    m = lemevit_amd.create_model("lemevit_tiny", num_classes=10).to(DEV).train()
    return m, lemevit_amd.FlatAdamW(m, lr=1e-3, eps=1e-3, weight_decay=0.05, **kw)


@functools.lru_cache(maxsize=None)
def _batch():
    return det_tensor((4, 3, 64, 64), "clip.img", 1).to(DEV), torch.tensor([3, 8, 1, 6], device=DEV)


def _backward(m, opt):
    x, y = _batch()
    opt.zero_grad(set_to_none=True)
    with torch.autocast("cuda", torch.bfloat16):
        loss = torch.nn.functional.cross_entropy(m(x), y)
    loss.backward()


def _params(m):
    return {n: p.detach().clone() for n, p in m.named_parameters()}


def _feed(src, dst):
    """clones of src's gradients become dst's (in place where dst's gradient is a view of a flat buffer)"""
    table = dict(src.named_parameters())
    for n, q in dst.named_parameters():
        g = table[n].grad
        if g is None:
            q.grad = None
        elif getattr(q, "_lmv_flat_grad", False):
            q.grad.copy_(g)
        else:
            q.grad = g.detach().clone()


@functools.lru_cache(maxsize=None)
def layer_case():
    """Computed once, read by the tests below.  A: FlatAdamW(layer_decay=0.75), three steps of its own forward / backward.  B: a deep copy of the initial model
    stepped by torch.optim.AdamW with one group per parameter (lr = 1e-3 * decay ** (L + 1 - id), weight decay 0 for ndim <= 1), fed clones of A's gradients on
    every step.  C: a plain FlatAdamW twin fed the same gradients.  A2: a second run of A."""
    from lemevit_amd import optim
    decay = 0.75
    ma, oa = _twin(layer_decay=decay)
    mc, oc = _twin()
    import lemevit_amd
    torch.manual_seed(0)
    mb = lemevit_amd.create_model("lemevit_tiny", num_classes=10).to(DEV).train()          # the twins' initial weights (asserted below)
    ids = optim.layer_ids(mb)
    L = 15
    assert max(ids.values()) == L + 1
    ob = torch.optim.AdamW([dict(params=[p], lr=1e-3 * decay ** (L + 1 - ids[n]), weight_decay=0.0 if p.ndim <= 1 else 0.05) for n, p in mb.named_parameters()],
                           betas=(0.9, 0.999), eps=1e-3)
    start = _params(ma)
    assert all(torch.equal(start[n], q) for n, q in _params(mb).items())
    for _ in range(3):
        _backward(ma, oa)
        _feed(ma, mb)
        oc.zero_grad()
        _feed(ma, mc)
        oa.step(); ob.step(); oc.step()
    m2, o2 = _twin(layer_decay=decay)
    for _ in range(3):
        _backward(m2, o2)
        o2.step()
    return dict(A=_params(ma), B=_params(mb), C=_params(mc), A2=_params(m2), start=start, flat={n for n, _, _, _ in oa._slices},
                groups=[(g["name"], g["lr"], g["lr_scale"], g["weight_decay"], len(g["params"])) for g in oa.param_groups], nflat=len(oa._flat_groups),
                hyper=oa._hyper.cpu(), step=oa.state_dict()["step"])


def test_layer_decay_matches_torch_adamw_with_one_group_per_parameter():
    """Every parameter within 1e-6 max(1, |p|max) (the clipping test's bound: three steps of at most a few lr each, rounding differences ~1e-7); the control -- the
    plain optimizer on the same gradients -- is further than that on the first block and on the stem; two runs are bit-identical."""
    case = layer_case()
    pa, pb, pc = case["A"], case["B"], case["C"]
    worst = max((float((pa[n] - pb[n]).abs().max()) / max(1.0, float(pb[n].abs().max())), n) for n in pa)
    print(f"layer_decay 0.75, A vs torch: worst parameter difference {worst[0]:.3e} of max(1, |p|max) at {worst[1]}; {case['nflat']} flat groups, {len(case['groups'])} in all")
    assert case["step"] == 3 and any(not torch.equal(pa[n], case["start"][n]) for n in pa)
    for n in pa:
        d = float((pa[n] - pb[n]).abs().max())
        assert d <= 1e-6 * max(1.0, float(pb[n].abs().max())), f"{n}: {d:.3e}"
    far = {n for n in pa if float((pa[n] - pc[n]).abs().max()) > 1e-6 * max(1.0, float(pc[n].abs().max()))}
    assert any(n.startswith("stages.0.0.") for n in far) and any(n.startswith("downsample_layers.0.") for n in far), "control: the plain twin must differ"
    assert any(n.startswith("stages.0.0.") for n in case["flat"]) and not any(n.startswith("downsample_layers.") for n in case["flat"])
    assert all(torch.equal(pa[n], case["A2"][n]) for n in pa)


def test_layer_decay_param_groups():
    """One dict per non-empty (scale, decays or not) group, the flat ones first; lr = base rate * lr_scale; the device table holds what the dicts say."""
    case = layer_case()
    groups, nflat = case["groups"], case["nflat"]
    assert nflat == 30 and all(name.startswith("blocks.") for name, *_ in groups[:nflat]) and all(name.startswith("rest.") for name, *_ in groups[nflat:])
    assert len({name for name, *_ in groups}) == len(groups) and all(k > 0 for *_, k in groups)
    for name, lr, scale, wd, _ in groups:
        assert lr == 1e-3 * scale and wd == (0.05 if name.endswith("_decay") and not name.endswith("no_decay") else 0.0)
    assert groups[0][2] == 0.75 ** 15 and any(scale == 1.0 for _, _, scale, _, _ in groups[nflat:])
    want = torch.tensor([[lr, wd] for _, lr, _, wd, _ in groups[:nflat]], dtype=torch.float32)
    assert torch.equal(case["hyper"], want)


def test_unit_scales_equal_the_plain_optimizer_bit_for_bit():
    """FlatAdamW(lr_scale=lambda n, p: 1.0) is table mode with unit scales: parameters (block and non-block), both moments and the bf16 copies end where the plain
    optimizer's end."""
    m1, o1 = _twin(lr_scale=lambda n, p: 1.0)
    m2, o2 = _twin()
    assert o1._hyper is not None and o1._wd_mask is None and o2._hyper is None
    for _ in range(3):
        _backward(m1, o1); o1.step()
        _backward(m2, o2); o2.step()
    p1, p2 = _params(m1), _params(m2)
    diff = [n for n in p1 if not torch.equal(p1[n], p2[n])]
    assert not diff, f"{len(diff)} parameters differ, e.g. {diff[:3]}"
    assert torch.equal(o1._exp_avg, o2._exp_avg) and torch.equal(o1._exp_avg_sq, o2._exp_avg_sq) and torch.equal(o1._shadow, o2._shadow)
    assert all(torch.equal(a, b) for (_, a), (_, b) in zip(o1._tpairs, o2._tpairs))
    assert o1.state_dict()["step"] == o2.state_dict()["step"] == 3


# ---- 5. a scheduled rate under capture ----------------------------------------------------------------------------------------------------------
R = 2.0 ** -10          # and its halves: exact in float32, so the float32 device rate a captured step reads IS the host rate an eager step hands torch's update


def _set_rate(opt, value):
    for g in opt.param_groups:          # what a timm-style scheduler does
        g["lr"] = value * g["lr_scale"]


@pytest.mark.parametrize("clip", [None, 1.0])
def test_scheduled_rate_under_graph_capture(clip):
    """Eager: three steps at rates r, r / 2, r / 4 written into param_groups.  Captured: one eager warm-up step at r, then two replays with the same writes ahead
    of each, uploaded by before_replay=opt.sync_hyper.  Bit-identical parameters, step count 3.  Control: the same replays without before_replay keep the rate
    of the capture and end elsewhere.  clip = 1.0 is the clipping tests' "small" threshold (below the gradient norm of every step): the device coefficient and
    the device rates coexist."""
    from lemevit_amd.graph import GraphedStep
    kw = dict(device_lr=True) if clip is None else dict(device_lr=True, clip_grad=clip)
    ma, oa = _twin(**kw)
    for k in range(3):
        _set_rate(oa, R * 0.5 ** k)
        _backward(ma, oa)
        oa.step()
        if clip is not None:
            assert float(oa._stat[1]) < 1.0, "clipping must be active"
    want = _params(ma)
    ends = {}
    for follow in (True, False):
        mb, ob = _twin(**kw)
        _set_rate(ob, R)
        g = GraphedStep(lambda: (_backward(mb, ob), ob.step()), warmup=1, before_replay=ob.sync_hyper if follow else None)
        for k in (1, 2):
            _set_rate(ob, R * 0.5 ** k)
            g()
        torch.cuda.synchronize()
        ops().check_stage_errors("graph replay", sync=False)
        assert ob.state_dict()["step"] == 3
        ends[follow] = _params(mb)
    diff = [n for n in want if not torch.equal(want[n], ends[True][n])]
    assert not diff, f"{len(diff)} parameters differ between the eager and the captured schedule, e.g. {diff[:3]}"
    flat = {n for n, _, _, _ in oa._slices}
    stale = {n for n in want if not torch.equal(want[n], ends[False][n])}
    assert stale & flat and stale - flat, "control: replays that never upload the rates must end elsewhere, on block and non-block parameters"


# ---- 6. bookkeeping -----------------------------------------------------------------------------------------------------------------------------
def test_state_dict_round_trip_and_defaults():
    m1, o1 = _twin(layer_decay=0.75)
    _backward(m1, o1)
    o1.step()
    for g in o1.param_groups:
        g["lr"] = 0.5e-3 * g["lr_scale"]
    o1.param_groups[0]["weight_decay"] = 0.02
    sd = o1.state_dict()
    assert sd["step"] == 1 and [g["name"] for g in sd["groups"]] == [g["name"] for g in o1.param_groups]
    assert set(sd["groups"][0]) == {"name", "lr", "lr_scale", "weight_decay"} and sd["lr"] == pytest.approx(0.5e-3, rel=1e-12)
    assert all(isinstance(g["lr"], float) for g in sd["rest"]["param_groups"])
    m2, o2 = _twin(layer_decay=0.75)
    o2.load_state_dict(sd)
    assert [(g["lr"], g["weight_decay"]) for g in o2.param_groups] == [(g["lr"], g["weight_decay"]) for g in o1.param_groups]
    assert torch.equal(o2._exp_avg, o1._exp_avg) and torch.equal(o2._exp_avg_sq, o1._exp_avg_sq) and o2.state_dict()["step"] == 1
    o1.sync_hyper()
    assert torch.equal(o2._hyper, o1._hyper) and float(o2._hyper[0, 1]) == torch.tensor(0.02).item()
    r1, r2 = o1._rest.state_dict()["state"], o2._rest.state_dict()["state"]
    assert all(torch.equal(r1[k]["exp_avg"], r2[k]["exp_avg"]) for k in r1)
    # a dict written without the group list: the scalar rate, this optimizer's scales
    legacy = {k: v for k, v in sd.items() if k != "groups"}
    m3, o3 = _twin(layer_decay=0.75)
    o3.load_state_dict(legacy)
    assert all(g["lr"] == pytest.approx(0.5e-3 * g["lr_scale"], rel=1e-12) for g in o3.param_groups) and torch.equal(o3._exp_avg, o1._exp_avg)
    # no new option: nothing of the table exists, and param_groups is what it was (the flat group + torch's two)
    m4, o4 = _twin()
    assert o4._hyper is None and o4._group_of_unit is None and o4._wd_mask is not None and len(o4.param_groups) == 3
    assert o4.param_groups[1] is o4._rest.param_groups[0]
    o4.sync_hyper()                                                      # nothing to upload: a no-op
    assert "groups" not in o4.state_dict()


def test_sync_hyper_uploads_only_after_a_change(monkeypatch):
    m, o = _twin(device_lr=True)
    calls = []
    real = torch.Tensor.copy_

    def spy(self, *a, **k):
        if self is o._hyper_dev:
            calls.append(1)
        return real(self, *a, **k)
    monkeypatch.setattr(torch.Tensor, "copy_", spy)
    o.sync_hyper()
    assert not calls, "nothing changed since the constructor's upload"
    _set_rate(o, 3e-4)
    o.sync_hyper(); o.sync_hyper()
    assert len(calls) == 1 and float(o._hyper[0, 0]) == torch.tensor(3e-4).item()
    assert len(o.param_groups) == 4 and [g["lr_scale"] for g in o.param_groups] == [1.0] * 4


def test_lr_scale_by_prefix_and_refusals():
    """An mmcv-style lr_mult by name prefix: a frozen prefix (scale 0) stays where it is, bit for bit, the others move; bad scales and more groups than the
    device table holds are refused."""
    import lemevit_amd
    frozen = ("stages.0.", "downsample_layers.0.")
    m, o = _twin(lr_scale=lambda n, p: 0.0 if n.startswith(frozen) else (0.1 if n.startswith("stages.1.") else 1.0))
    assert sorted({g["lr_scale"] for g in o.param_groups}) == [0.0, 0.1, 1.0]
    before = _params(m)
    _backward(m, o)
    o.step()
    after = _params(m)
    assert all(torch.equal(before[n], after[n]) for n in before if n.startswith(frozen))
    for n in ("stages.1.0.mlp.0.weight", "stages.3.0.attn.qkv.weight", "head.weight", "downsample_layers.2.0.weight"):
        assert not torch.equal(before[n], after[n]), n
    for bad in (float("nan"), float("inf"), -1.0):
        with pytest.raises(ValueError, match="scale"):
            lemevit_amd.FlatAdamW(m, lr_scale=lambda n, p: bad)
    cfg = dict(depth=[2, 2, 2, 10, 4], embed_dim=[64, 64, 128, 192, 320], head_dim=32, attn_type=["C", "D", "D", "S", "S"], queries_len=16)
    deep = lemevit_amd.LeMeViT(num_classes=10, **cfg).to(DEV)
    count = iter(range(10 ** 6))
    with pytest.raises(ValueError, match="device table holds 256"):
        lemevit_amd.FlatAdamW(deep, lr_scale=lambda n, p: 1.0 + next(count))
