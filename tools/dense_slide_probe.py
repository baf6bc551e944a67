"""Sliding-window dense inference in one pass (lmv_dense_slide_fwd: stitch, resize and argmax without the full-resolution maps) against mmseg's loop in stock
PyTorch on the GPU (GPU box).

    python tools/dense_slide_probe.py [--calls 20] [--rounds 5] [--out profiles/dense_slide_probe.txt]

The same stack of window logits [G, 1, 6, 128, 128] (crop 512, stride 384, a 4 x head) is stitched by
    fused   dense.slide_predict / SegMeter.update_slide (one / two launches);
    stock   the literal loop: per window F.interpolate to the crop, F.pad to the image, `preds +=`, `count_mat +=`; then `/`, argmax (and, for the meter's
            side, F.cross_entropy with ignore_index + bincount + the histogram's copy to the host).
Two tiles: 1536 x 1536 (16 windows) and the Potsdam tile 6000 x 6000 (256 windows), the largest the reference's data holds.  Windows of --calls calls between
device events in one process, --rounds windows per side, the sides alternating; median and spread (max - min) reported, and torch.cuda.max_memory_allocated of
one call above what was allocated before it (the stack and the labels are inputs of both sides)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from lemevit_amd import dense
from dense_loss_probe import LINES, compare, say
from dense_up_probe import peak_mb


def stock_loop(x, grid):
    G, B, K = x.shape[:3]
    preds = x.new_zeros((B, K, grid.H, grid.W))
    count_mat = x.new_zeros((B, 1, grid.H, grid.W))
    for g, (y1, y2, x1, x2) in enumerate(grid.boxes()):
        crop_seg_logit = F.interpolate(x[g], size=(y2 - y1, x2 - x1), mode="bilinear", align_corners=False)
        preds += F.pad(crop_seg_logit, (x1, grid.W - x2, y1, grid.H - y2))
        count_mat[:, :, y1:y2, x1:x2] += 1
    return preds / count_mat


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="+", default=[1536, 6000])
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "dense_slide_probe.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dense_slide_probe: needs an MI355X (no CPU fallback)")
    torch.manual_seed(0)
    dev, K, ignore = "cuda", 6, 255
    say(f"dense_slide_probe: {torch.cuda.get_device_name(0)}, medians of {a.rounds} windows of {a.calls} calls")
    with torch.no_grad():
        for S in a.sizes:
            grid = dense.slide_grid((S, S), 512, 384)
            G = len(grid)
            x = torch.randn(G, 1, K, 128, 128, device=dev) * 3
            y = torch.randint(0, K, (1, S, S), device=dev)
            y[torch.rand(1, S, S, device=dev) < 0.2] = ignore
            y8, yflat = y.to(torch.uint8), y.reshape(-1)
            say(f"--- {S} x {S}, K = {K}, crop 512, stride 384: {G} windows, window logits [{G}, 1, {K}, 128, 128] fp32 ({x.numel() * 4 / 1e6:.1f} MB); "
                f"the full-resolution map {K * S * S * 4 / 1e6:.1f} MB, uint8 labels {S * S / 1e6:.1f} MB")
            meter = dense.SegMeter(K, ignore_index=ignore)
            meter.update_slide(x, grid, y8)

            def stock_pred():
                return stock_loop(x, grid).argmax(1)

            def stock_meter():
                z = stock_loop(x, grid)
                loss = F.cross_entropy(z, y, ignore_index=ignore)
                pred = z.argmax(1).reshape(-1)
                on = yflat != ignore
                return loss, torch.bincount(yflat[on] * K + pred[on], minlength=K * K).reshape(K, K).cpu()

            sides_p = [("fused: slide_predict (one launch)", lambda: dense.slide_predict(x, grid)), ("stock: the literal loop + argmax", stock_pred)]
            sides_m = [("fused: SegMeter.update_slide (two launches, no synchronisation)", lambda: meter.update_slide(x, grid, y8)),
                       ("stock: the literal loop + cross_entropy + argmax + bincount + the histogram's copy to the host", stock_meter)]
            compare("prediction", sides_p, a.calls, a.rounds)
            say("  peak memory of one call above what was allocated before it: " + ", ".join(f"{n} {peak_mb(f):.1f} MB" for n, (_, f) in zip(("fused", "stock"), sides_p)))
            compare("prediction + loss + confusion matrix", sides_m, a.calls, a.rounds)
            say("  peak memory of one call above what was allocated before it: " + ", ".join(f"{n} {peak_mb(f):.1f} MB" for n, (_, f) in zip(("fused", "stock"), sides_m)))
            pf, ps = dense.slide_predict(x, grid), stock_pred()
            meter.reset()
            meter.update_slide(x, grid, y8)
            loss_s, conf_s = stock_meter()
            m = meter.compute()
            say(f"  agreement: {int((pf.long() != ps).sum())} of {ps.numel()} predictions differ; loss fused {m['loss']:.7f}, stock {float(loss_s):.7f}; "
                f"{int((meter.conf.cpu() != conf_s).sum())} of {K * K} confusion cells differ")
            del x, y, y8, yflat, pf, ps, meter
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
