"""Two builds of the library, bit for bit, on the dense losses (GPU box): every output of lmv_dense_loss_fwd / _bwd and lmv_dense_up_loss_fwd / _bwd over the case
lists of tests/test_dense_loss_gpu.py and tests/test_dense_up_gpu.py -- both logits dtypes, both label dtypes, both layouts, every mode, ``pred``, ``conf`` and
``meter`` on.

    python tools/dense_ab.py LIB_A LIB_B [--timeout 600] [--out profiles/NAME.txt]

For each library a FRESH child process (``LMV_LIB_PATH`` names the build it loads; this process never opens the GPU), one after the other, each under its own time
limit; a child that fails ends the run before the next one starts.  A child writes one line per case with a digest of the bytes of ``stats, pred, conf, meter,
dlogits``; this process compares the two files, prints one line per case and the count of differing outputs, and exits 1 unless that count is 0."""
import argparse
import hashlib
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUTPUTS = ("stats", "pred", "conf", "meter", "dlogits")


def digest(t):
    import torch
    t = t.contiguous()
    return hashlib.blake2b((t.view(torch.int16) if t.dtype == torch.bfloat16 else t).cpu().numpy().tobytes(), digest_size=12).hexdigest()


def child(path):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import torch
    import test_dense_loss_gpu as tn
    import test_dense_up_gpu as tu
    from lemevit_amd import ops

    def run(f, name, fwd, bwd, x, y, K, npix, kw, gout):
        okw = tn.op_kwargs(kw, K)
        gt = None if gout is None else torch.tensor(gout, dtype=torch.float32, device=tn.DEV)
        pred = torch.full((x.shape[0], npix), 77, dtype=torch.uint8, device=tn.DEV)
        conf = torch.zeros((K, K), dtype=torch.int64, device=tn.DEV)
        meter = torch.zeros(2, dtype=torch.float64, device=tn.DEV)
        stats = fwd(x, y, pred=pred, conf=conf, meter=meter, **okw)
        dl = bwd(x, y, stats, gout=gt, **okw)
        f.write(name + "\t" + " ".join(digest(t) for t in (stats, pred, conf, meter, dl)) + "\n")

    kinds = [(d, l, lay) for d in (torch.float32, torch.bfloat16) for l in (torch.int64, torch.uint8) for lay in ("contiguous", "view")]
    with open(path, "w") as f:
        for shape in tn.SHAPES:
            for dtype, ldtype, layout in kinds:
                x32, y = tn.inputs(shape, ldtype)
                xd, yd = tn.on_device(x32.to(dtype), layout), y.to(tn.DEV)
                for mode, kw in tn.modes(shape[1]):
                    run(f, f"native {'x'.join(map(str, shape))} {dtype} {ldtype} {layout} {mode}".replace("torch.", ""), ops.dense_loss_fwd, ops.dense_loss_bwd,
                        xd, yd, shape[1], shape[2] * shape[3], kw, None)
        for case in tu.CASES:
            shape, size, align = case
            for dtype, ldtype, layout in kinds:
                x32, y = tu.inputs(shape, size, ldtype)
                xd, yd = tu.on_device(x32.to(dtype), layout), y.to(tn.DEV)
                for mode, kw, gout in tu.modes(shape[1]):
                    run(f, f"up {tu.case_id(case)} {dtype} {ldtype} {layout} {mode}".replace("torch.", ""),
                        lambda x, y, **k: ops.dense_up_loss_fwd(x, y, align, **k), lambda x, y, st, **k: ops.dense_up_loss_bwd(x, y, st, align, **k),
                        xd, yd, shape[1], size[0] * size[1], kw, gout)
        torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("libs", nargs="*")
    ap.add_argument("--child", help="(internal) write the digests of the library in LMV_LIB_PATH to this file")
    ap.add_argument("--timeout", type=int, default=600, help="seconds per child")
    ap.add_argument("--out", help="also write the report here")
    a = ap.parse_args()
    if a.child:
        return child(a.child)
    if len(a.libs) != 2:
        ap.error("two library paths expected")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    files = []
    with tempfile.TemporaryDirectory() as tmp:
        for side, lib in zip("AB", a.libs):
            out = os.path.join(tmp, side + ".txt")
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", out], env=dict(os.environ, LMV_LIB_PATH=os.path.abspath(lib)),
                                timeout=a.timeout).returncode
            if rc != 0:
                raise SystemExit(f"dense_ab: the child of library {side} ended with status {rc}; nothing more is run")
            files.append(dict(line.rstrip("\n").split("\t") for line in open(out)))
    A, B = files
    say(f"dense_ab: {len(A)} cases, outputs {', '.join(OUTPUTS)}; A = the first library, B = the second")
    differ = len(set(A) ^ set(B))
    for name in A:
        if name not in B:
            say(f"{name}: missing from B")
            continue
        bad = [o for o, x, y in zip(OUTPUTS, A[name].split(), B[name].split()) if x != y]
        differ += len(bad)
        say(f"{name}: " + ("equal" if not bad else "DIFFER: " + ", ".join(bad)))
    say(f"differing outputs: {differ}")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if differ == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
