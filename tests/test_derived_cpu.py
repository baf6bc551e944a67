"""The host-side caches of the model on CPU tensors: model.derived (every operand the kernels read instead of the parameters themselves),
LeMeBlock._params(), the DropPath keep vector and ModelEma's source tensors.  tests/test_derived_gpu.py runs the same rules through the model."""
import gc
import weakref

import pytest
import torch

import lemevit_amd as L
import lemevit_amd.model as M


class _Owner:
    pass


class _Counter:
    def __init__(self):
        self.n = 0

    def __call__(self):
        self.n += 1
        return torch.full((2,), float(self.n))


def test_derived_builds_once_while_nothing_changes():
    owner, p = _Owner(), torch.nn.Parameter(torch.ones(3))
    build = _Counter()
    with torch.no_grad():
        first = M.derived(owner, "t", (p, None), build)
        for _ in range(3):
            assert M.derived(owner, "t", (p, None), build) is first
    assert build.n == 1
    assert M.derived(owner, "other", (p, None), build) is not first and build.n == 2          # another tag is another entry


@pytest.mark.parametrize("change", ["in_place", "rehome", "training_pass", "replace_source", "grad_mode"])
def test_derived_rebuilds_after(change):
    owner, p, q = _Owner(), torch.nn.Parameter(torch.ones(3)), torch.zeros(3)
    src = [p, q]
    build = _Counter()
    with torch.no_grad():
        M.derived(owner, "t", src, build)
        if change == "in_place":
            q.add_(1.0)
        elif change == "rehome":
            p.data = torch.full((3,), 2.0)          # same Parameter object, same _version, new storage
        elif change == "training_pass":
            M.new_training_pass()
        elif change == "replace_source":
            src = [p, torch.zeros(3)]
    if change == "grad_mode":
        M.derived(owner, "t", src, build)          # grad enabled and p requires grad
    else:
        with torch.no_grad():
            M.derived(owner, "t", src, build)
    assert build.n == 2, change
    with torch.no_grad() if change != "grad_mode" else torch.enable_grad():
        M.derived(owner, "t", src, build)
    assert build.n == 2, change          # and then it is valid again


def test_derived_grad_mode_only_matters_for_sources_that_require_grad():
    owner, t = _Owner(), torch.ones(3)
    build = _Counter()
    with torch.no_grad():
        M.derived(owner, "t", (t,), build)
    M.derived(owner, "t", (t,), build)
    assert build.n == 1


def test_derived_entry_goes_with_its_owner():
    gc.collect()
    before = len(M._derived)
    owner, p = _Owner(), torch.ones(3)
    with torch.no_grad():
        M.derived(owner, "a", (p,), _Counter())
        M.derived(owner, "b", (p,), _Counter())
    assert len(M._derived) == before + 2
    ref = weakref.ref(owner)
    del owner
    gc.collect()
    assert ref() is None, "the cache keeps its owner alive"
    assert len(M._derived) == before
    # a source the cache built from is not kept alive either
    owner, p = _Owner(), torch.ones(3)
    with torch.no_grad():
        M.derived(owner, "a", (p,), _Counter())
    pref = weakref.ref(p)
    del p
    gc.collect()
    assert pref() is None, "the cache keeps a source alive"


def test_derived_counts_one_fill_per_build():
    owner, p = _Owner(), torch.ones(3)
    build = _Counter()
    f0 = M.cache_fills()
    with torch.no_grad():
        M.derived(owner, "t", (p,), build)
        M.derived(owner, "t", (p,), build)
        assert M.cache_fills() == f0 + 1
        p.mul_(2.0)
        M.derived(owner, "t", (p,), build)
        M.derived(owner, "t", (p,), build)
    assert build.n == 2 and M.cache_fills() == f0 + 2


def _live_params_match(m):
    for blk in (b for st in m.stages for b in st):
        live = dict(blk.named_parameters())
        got = blk._params()
        assert list(got) == list(M.PARAM_NAMES[blk.attn_type])
        for n, p in got.items():
            if p is not live[n]:
                return False
    return True


def test_block_params_follow_assign_load():
    m = L.create_model("lemevit_tiny", num_classes=10)
    assert _live_params_match(m)          # (fills every block's table)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    m.load_state_dict(sd, assign=True)
    assert _live_params_match(m), "LeMeBlock._params() returns the Parameters load_state_dict(assign=True) replaced"


def test_block_params_follow_apply_that_replaces_parameters():
    m = L.create_model("lemevit_tiny", num_classes=10)
    assert _live_params_match(m)
    was = torch.__future__.get_overwrite_module_params_on_conversion()
    torch.__future__.set_overwrite_module_params_on_conversion(True)          # .to() then builds new Parameter objects
    try:
        m.to(torch.float64)
    finally:
        torch.__future__.set_overwrite_module_params_on_conversion(was)
    assert _live_params_match(m)


def _keep_vector(m, device):
    m._draw_drop_path(3, device)
    return m._dp_keep[1]


def test_drop_path_keep_vector_follows_rates():
    torch.manual_seed(0)
    m = L.create_model("lemevit_tiny", num_classes=10, drop_path_rate=0.1).train()
    dev = torch.device("cpu")
    k0 = _keep_vector(m, dev)
    assert _keep_vector(m, dev) is k0, "unchanged rates: the device copy is reused (no upload per step)"
    blk = m.stages[3][2]
    blk.drop_prob = 0.5
    k1 = _keep_vector(m, dev)
    want = [1.0 - b.drop_prob for st in m.stages for b in st if b.drop_prob > 0.0 for _ in range(2 if b.kind in ("C", "Sx") else 4)]
    assert torch.equal(k1, torch.tensor(want, dtype=torch.float32)), "the keep vector ignores a changed drop_prob"
    assert 0.5 in k1.tolist()
    assert _keep_vector(m, dev) is k1


def test_model_ema_follows_rehomed_parameters():
    torch.manual_seed(0)
    m = L.create_model("lemevit_tiny", num_classes=10)
    decay = 0.75
    ema = L.ModelEma(m, decay=decay)
    ref = {k: v.detach().clone().double() for k, v in m.state_dict().items() if v.dtype.is_floating_point}

    def step(scale):
        with torch.no_grad():
            for p in m.parameters():
                p.data = p.detach() * scale + 0.01          # re-homed: new storage behind the same Parameter
        ema.update(m)
        for k, v in m.state_dict().items():
            if v.dtype.is_floating_point:
                ref[k] = decay * ref[k] + (1 - decay) * v.detach().double()

    ema.update(m)
    for k, v in m.state_dict().items():
        if v.dtype.is_floating_point:
            ref[k] = decay * ref[k] + (1 - decay) * v.detach().double()
    for s in (1.25, 0.5):
        step(s)
    got = ema.module.state_dict()
    for k, r in ref.items():
        assert torch.allclose(got[k].double(), r, rtol=1e-5, atol=1e-6), k
