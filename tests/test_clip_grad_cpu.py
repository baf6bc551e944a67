"""Host side of the native gradient clipping (lmv_grad_norm / lmv_adamw_flat_clip, include/lemevit_hip.h) without a GPU: the argument checks run before
any launch, and the workspace -- the partition of the reduction -- is a function of the segment lengths alone."""
import ctypes
import os

import pytest
import torch

ERR_SHAPE = -1
FAKE = 1 << 20          # a 16-byte aligned address that is never dereferenced: every call below is refused before a launch


def _table(lengths, ptr=FAKE):
    from lemevit_amd._lib import NormSeg
    arr = (NormSeg * len(lengths))()
    for sg, n in zip(arr, lengths):
        sg.ptr, sg.n = ptr, n
    return arr


def _refused(rc, word):
    from lemevit_amd._lib import lib
    msg = lib.lmv_last_error()
    assert rc == ERR_SHAPE and word in msg, (rc, msg)


def test_grad_norm_rejects_bad_arguments_before_any_launch():
    from lemevit_amd._lib import lib
    seg = _table([1000])
    need = lib.lmv_grad_norm_workspace_bytes(seg, 1)
    assert need == 4
    _refused(lib.lmv_grad_norm(None, 1, 1.0, 0, FAKE, None, FAKE, need, None), b"segs is NULL")
    _refused(lib.lmv_grad_norm(seg, 0, 1.0, 0, FAKE, None, FAKE, need, None), b"nsegs")
    _refused(lib.lmv_grad_norm(seg, 1, 1.0, 0, None, None, FAKE, need, None), b"stat")
    _refused(lib.lmv_grad_norm(seg, 1, 1.0, 0, FAKE + 4, None, FAKE, need, None), b"stat")
    _refused(lib.lmv_grad_norm(seg, 1, 1.0, 0, FAKE, None, FAKE, need - 1, None), b"workspace")
    _refused(lib.lmv_grad_norm(seg, 1, 1.0, 0, FAKE, None, None, need, None), b"workspace")
    _refused(lib.lmv_grad_norm(_table([-1]), 1, 1.0, 0, FAKE, None, FAKE, 64, None), b"negative length")
    _refused(lib.lmv_grad_norm(_table([8], ptr=FAKE + 2), 1, 1.0, 0, FAKE, None, FAKE, 64, None), b"4-byte aligned")
    _refused(lib.lmv_grad_norm(_table([8], ptr=0), 1, 1.0, 0, FAKE, None, FAKE, 64, None), b"null")
    assert lib.lmv_grad_norm_workspace_bytes(None, 1) == 0 and lib.lmv_grad_norm_workspace_bytes(seg, 0) == 0


def test_adamw_flat_clip_rejects_bad_arguments_before_any_launch():
    from lemevit_amd._lib import lib
    f = lib.lmv_adamw_flat_clip
    _refused(f(FAKE, FAKE, FAKE, FAKE, None, None, 6, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, None, None, 0.0, None), b"multiple of 4")
    _refused(f(FAKE, FAKE, FAKE, FAKE, None, None, 8, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0, None, None, 0.0, None), b"step")
    _refused(f(FAKE, None, FAKE, FAKE, None, None, 8, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, None, None, 0.0, None), b"null or misaligned")
    _refused(f(FAKE, FAKE, FAKE, FAKE, None, None, 8, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, None, FAKE + 2, 0.0, None), b"null or misaligned")
    _refused(f(FAKE, FAKE, FAKE, FAKE, None, None, 8, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, None, None, -1.0, None), b"clip_value")
    _refused(f(FAKE, FAKE, FAKE, FAKE, None, None, 8, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, None, None, float("nan"), None), b"clip_value")


def test_grad_norm_workspace_is_a_function_of_the_segment_lengths():
    """One fp32 partial per chunk of LMV_NORM_CHUNK elements, every segment cut on its own: the two lengths on either side of a chunk boundary, and the
    pointers do not enter."""
    from lemevit_amd import _lib, ops
    lib, CH = _lib.lib, ops.NORM_CHUNK
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "lemevit_hip.h")).read()
    assert f"#define LMV_NORM_CHUNK {CH}\n" in hdr and f"#define LMV_GRAD_STAT_FLOATS {ops.GRAD_STAT_FLOATS}\n" in hdr
    assert 16 * 1024 <= CH <= 64 * 1024

    def nbytes(lengths, ptr=FAKE):
        return lib.lmv_grad_norm_workspace_bytes(_table(lengths, ptr), len(lengths))
    assert nbytes([CH]) == 4 and nbytes([CH + 1]) == 8
    assert nbytes([1]) == 4 and nbytes([3 * CH]) == 12 and nbytes([3 * CH + 8]) == 16
    assert nbytes([CH, 1, CH + 1]) == 4 * (1 + 1 + 2)          # segments do not share a chunk
    assert nbytes([CH + 1] * 130) == 4 * 2 * 130               # more segments than one by-value table holds
    assert nbytes([CH + 1, 0, 7]) == 4 * 3                     # an empty segment has no chunk
    assert nbytes([CH + 1, 10], ptr=FAKE + 4) == nbytes([CH + 1, 10])


def test_ops_refuse_cpu_tensors_and_flat_adamw_refuses_unsupported_modes():
    from lemevit_amd import ops
    stat = torch.zeros(ops.GRAD_STAT_FLOATS)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.grad_norm([torch.ones(8)], 1.0, stat)
    with pytest.raises(TypeError, match="stat"):
        ops.grad_norm([torch.ones(8)], 1.0, torch.zeros(4))
    t = torch.zeros(8)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.adamw_flat(t, t, t, t, None, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, clip_value=0.5)
    import lemevit_amd
    m = torch.nn.Linear(2, 2)
    with pytest.raises(NotImplementedError, match="adaptive_clip_grad"):
        lemevit_amd.FlatAdamW(m, clip_grad=1.0, clip_mode="agc")
    with pytest.raises(ValueError, match="clip_mode"):
        lemevit_amd.FlatAdamW(m, clip_grad=1.0, clip_mode="l1")
    assert ctypes.sizeof(lemevit_amd._lib.NormSeg) == 16
