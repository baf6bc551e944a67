"""Image gradients and in_chans != 3 without a GPU: the two C-ABI entry points of csrc/conv1.hip refuse bad arguments before any launch, the oracle
meets the reference's fixtures (image gradient, logits, loss, first-conv weight gradient: the fp32 class of the project, 1e-5 of max-abs -- reference vs oracle measured
0.3 - 3.3e-6 here), the in_chans = N state_dict layout, and load_checkpoint's adaptation of an RGB checkpoint to an N-channel stem (timm's adapt_input_conv rule)."""
import numpy as np
import pytest
import torch

from detfill import det_tensor, fill_state_dict, sample
from oracle import lemevit_oracle as O

FIRST = "downsample_layers.0.0.weight"


def _close(out, ref, tol, what):
    out = np.asarray(out.detach().numpy() if torch.is_tensor(out) else out, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    assert out.shape == ref.shape, (what, out.shape, ref.shape)
    mx = max(np.abs(ref).max(), 1e-30)
    err = np.abs(out - ref).max() / mx
    print(f"{what}: rel max-abs err {err:.2e}")
    assert err <= tol, f"{what}: {err:.3e} > {tol:.0e} of max-abs {mx:.3e}"


def test_entry_points_refuse_bad_arguments():
    from lemevit_amd import _lib
    lib = _lib.lib
    assert {"lmv_im2col3x3s2_nchw", "lmv_conv3x3s2_nchw_dx"} <= set(_lib.SIGNATURES) and _lib.ABI_VERSION >= 13
    p = 1 << 20          # (a non-null, aligned address: no launch happens on any of these calls)

    def im2col(x=p, xd=0, out=p, d=1, B=2, Cin=4, H=8, W=8, KP=64):
        return lib.lmv_im2col3x3s2_nchw(x, xd, out, d, B, Cin, H, W, KP, Cin * H * W, H * W, W, 1, None)

    def dx(dy=p, wm=p, out=p, od=0, B=2, Cin=4, H=8, W=8, Co=48, KP=64, d=1):
        return lib.lmv_conv3x3s2_nchw_dx(dy, wm, out, od, B, Cin, H, W, Co, KP, Cin * H * W, H * W, W, 1, d, None)

    for fn, name, bad in [(im2col, b"im2col3x3s2_nchw", [dict(x=None), dict(out=None)]), (dx, b"conv3x3s2_nchw_dx", [dict(dy=None), dict(wm=None), dict(out=None), dict(Co=0), dict(Co=12)])]:
        for kw in bad + [dict(Cin=0), dict(B=0), dict(H=0), dict(KP=32), dict(KP=40), dict(KP=72)]:
            assert fn(**kw) == -1 and name in lib.lmv_last_error(), (name, kw, lib.lmv_last_error())
        assert fn(d=7) == -2 and name in lib.lmv_last_error()
    assert im2col(xd=5) == -2 and dx(od=3) == -2
    assert dx(dy=p + 8) == -1 and b"misaligned" in lib.lmv_last_error()
    assert dx(B=1 << 12, H=1 << 10, W=1 << 10) == -1 and b"2^31" in lib.lmv_last_error()


def _oracle_step(meta, name, train=True):
    cfg = O.VARIANTS[meta["variant"]]
    cin = meta.get("in_chans", 3)
    sd = fill_state_dict(O.state_dict_spec(cfg, meta["num_classes"], in_chans=cin), meta["seed"])
    for k, v in sd.items():
        if v.dtype.is_floating_point and not k.endswith(("running_mean", "running_var")):
            v.requires_grad_(True)
    img = det_tensor((meta["B"], cin, meta["res"], meta["res"]), meta.get("img", name + ".img"), 5).requires_grad_(True)
    stats = {}
    logits = O.lemevit_forward(sd, cfg, img, train=train, new_stats=stats)
    return sd, img, logits, stats


def test_oracle_image_gradient_train(golden):
    meta, g = golden("inputgrad_tiny_96")
    _, t = golden("train_tiny_96")
    sd, img, logits, _ = _oracle_step(meta, "inputgrad_tiny_96")
    loss = torch.nn.functional.cross_entropy(logits, torch.tensor(meta["target"]))
    loss.backward()
    assert float(g["loss"]) == float(t["loss"]) and np.array_equal(g["grad." + FIRST], t["grad." + FIRST]), "the reference's step does not depend on requires_grad of the image"
    _close(logits.detach(), t["logits"], 1e-5, "logits")
    assert abs(loss.item() - float(g["loss"])) <= 1e-5 * max(1.0, abs(float(g["loss"])))
    _close(img.grad, g["dimg"], 1e-5, "dimg")
    _close(sd[FIRST].grad, g["grad." + FIRST], 1e-5, "grad " + FIRST)


def test_oracle_image_gradient_eval(golden):
    meta, g = golden("inputgrad_tiny_96_eval")
    _, img, logits, _ = _oracle_step(meta, "inputgrad_tiny_96_eval", train=False)
    logits[:, torch.tensor(meta["target"])].sum().backward()
    _close(logits.detach(), g["logits"], 1e-5, "logits")
    _close(img.grad, g["dimg"], 1e-5, "dimg")


@pytest.mark.parametrize("name", ["train_tiny_c4_96", "train_tiny_c13_96"])
def test_oracle_in_chans_train_step(golden, name):
    meta, g = golden(name)
    sd, img, logits, stats = _oracle_step(meta, name)
    loss = torch.nn.functional.cross_entropy(logits, torch.tensor(meta["target"]))
    loss.backward()
    _close(logits.detach(), g["logits"], 1e-5, "logits")
    assert abs(loss.item() - float(g["loss"])) <= 1e-5 * max(1.0, abs(float(g["loss"])))
    gn = np.array([float(sd[k].grad.norm()) if sd[k].grad is not None else 0.0 for k in meta["param_names"]], dtype=np.float32)
    assert np.all(np.abs(gn - g["grad_norms"]) <= 3e-4 * np.maximum(1.0, np.abs(g["grad_norms"]))), np.abs(gn - g["grad_norms"]).max()
    _close(sd[FIRST].grad, g["grad." + FIRST], 1e-5, "grad " + FIRST)
    _close(sample(img.grad, meta["dimg_sampled"]) if meta["dimg_sampled"] else img.grad, g["dimg"], 1e-5, "dimg")
    for k in g:
        if k.startswith("stat."):
            _close(stats[k[5:]], g[k], 1e-5, k)


def test_oracle_one_channel_forward(golden):
    meta, g = golden("model_tiny_c1_224")
    cfg = O.VARIANTS[meta["variant"]]
    sd = fill_state_dict(O.state_dict_spec(cfg, meta["num_classes"], in_chans=1), meta["seed"])
    with torch.no_grad():
        logits = O.lemevit_forward(sd, cfg, det_tensor((1, 1, 224, 224), "model_tiny_c1_224.img", 4))
    _close(logits, g["logits"], 1e-5, "logits")


def test_in_chans_state_dict_layout():
    import lemevit_amd as L
    m = L.create_model("lemevit_tiny", num_classes=10, in_chans=4)
    spec = O.state_dict_spec(O.VARIANTS["lemevit_tiny"], 10, in_chans=4)
    sd = m.state_dict()
    assert list(sd.keys()) == list(spec.keys())
    assert all(tuple(sd[k].shape) == tuple(spec[k]) for k in sd) and tuple(sd[FIRST].shape) == (32, 4, 3, 3)


@pytest.mark.parametrize("prefix", ["", "module.backbone."])
def test_load_rgb_checkpoint_into_n_channel_model(tmp_path, prefix):
    import lemevit_amd as L
    src = L.create_model("lemevit_tiny", num_classes=10)
    src.load_state_dict(fill_state_dict({k: tuple(v.shape) for k, v in src.state_dict().items()}, 9))
    path = str(tmp_path / "rgb.pth")
    torch.save({"model": {prefix + k: v for k, v in src.state_dict().items()}}, path)
    w = src.state_dict()[FIRST]
    for n in (1, 4, 13):
        want = w.sum(dim=1, keepdim=True) if n == 1 else w.repeat(1, (n + 2) // 3, 1, 1)[:, :n] * (3.0 / n)
        m = L.create_model("lemevit_tiny", num_classes=10, in_chans=n, checkpoint_path=path)
        got = m.state_dict()
        assert got[FIRST].shape == (32, n, 3, 3) and torch.equal(got[FIRST], want)
        assert all(torch.equal(got[k], v) for k, v in src.state_dict().items() if k != FIRST)
    assert torch.equal(got[FIRST][:, 3], w[:, 0] * (3.0 / 13)) and torch.equal(got[FIRST][:, 11], w[:, 2] * (3.0 / 13))          # (n = 13) channel i = checkpoint channel i % 3, scaled
    same = L.create_model("lemevit_tiny", num_classes=10, checkpoint_path=path)          # same-shape load: untouched
    assert all(torch.equal(v, same.state_dict()[k]) for k, v in src.state_dict().items())
    bb = L.LeMeViTBackbone(in_chans=4, depth=[1, 2, 2, 8, 2], embed_dim=[64, 64, 128, 192, 320], head_dim=32, attn_type=["C", "D", "D", "S", "S"], queries_len=16)
    bb.init_weights(path)
    assert torch.equal(bb.state_dict()[FIRST], w.repeat(1, 2, 1, 1)[:, :4] * 0.75)
