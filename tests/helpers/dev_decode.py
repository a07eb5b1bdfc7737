"""TEST INFRASTRUCTURE -- a batch decoded from HBM to HBM (zk_decode_frames_dev) under a pinned ZK_CHOICE_ENTROPY, for the tests of the fused
entropy kernel (tests/test_gpu_entropy_fused.py, tests/test_gpu_generated_variants.py)."""
import numpy as np


def dev():
    import torch
    return torch.device("cuda", 0)


def upload(comp, c, d):
    """-> (compressed bytes + 64 of padding, their count, compressed offsets, decoded offsets), all on the device"""
    import torch
    return (torch.from_numpy(np.frombuffer(bytes(comp) + b"\0" * 64, np.uint8).copy()).to(dev()), len(comp),
            torch.from_numpy(np.asarray(c, np.uint64).view(np.int64).copy()).to(dev()), torch.from_numpy(np.asarray(d, np.uint64).view(np.int64).copy()).to(dev()))


def decode(engine, setting, arch, nf, total, d_out=None, poison=0, verify=True):
    """-> (rc, output tensor, statuses, whether the fused kernel ran) with ZK_CHOICE_ENTROPY = setting; the output buffer is filled with
    `poison` and the statuses with -1 before the call"""
    import torch
    d_comp, csize, d_c, d_d = arch
    if d_out is None:
        d_out = torch.empty(total + 64, dtype=torch.uint8, device=dev())
    d_out.fill_(poison)
    d_st = torch.full((nf,), -1, dtype=torch.int32, device=dev())
    engine.set_kernel_choice(reset=0)
    try:
        engine.set_kernel_choice(entropy=setting)
        rc = engine.decode_frames_dev(d_comp, csize, d_c, d_d, 0, nf, d_out, total, verify, d_st)
        fused = engine.entropy_fused()
    finally:
        engine.set_kernel_choice(reset=0)
    torch.cuda.synchronize()
    return rc, d_out, d_st.cpu().numpy(), fused


def both(engine, arch, nf, total, same_bytes=True, poison=0):
    """the batch under ZK_CHOICE_ENTROPY = 1 and = 2: the same return code and statuses (and bytes) -> what `decode` returns for 2"""
    import torch
    rc1, o1, st1, f1 = decode(engine, 1, arch, nf, total, poison=poison)
    rc2, o2, st2, f2 = decode(engine, 2, arch, nf, total, poison=poison)
    assert not f1, "ZK_CHOICE_ENTROPY = 1 is the two kernels"
    assert rc1 == rc2 and np.array_equal(st1, st2)
    if same_bytes:
        assert torch.equal(o1[:total], o2[:total])
    return rc2, o2, st2, f2
