"""What the segment-launch GPU tests (test_td3_segments_gpu / test_dueling_segments_gpu / test_ppo_segments_gpu) share: a snapshot of an
inner loop's outputs, the bit comparison of two snapshots, the runners of a single launch and of a series of segments, and the hook that
poisons the outputs of finished chains."""
import numpy as np
import torch

SENTINEL = 77


def snapshot(il, names):
    """Host copies of the outputs `names`, of every trace array (as trace_<name>) and, for an ICM agent, of icm_final (synchronises)."""
    torch.cuda.synchronize()
    out = {k: getattr(il, k).cpu().numpy().copy() for k in names}
    out.update({"trace_" + k: v.cpu().numpy().copy() for k, v in il.trace.items()})
    if getattr(il, "icm", False):
        out["icm_final"] = il.icm_final.cpu().numpy().copy()
    return out


def same_bits(a, b, what):
    assert sorted(a) == sorted(b), what
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, (what, k)
        assert a[k].tobytes() == b[k].tobytes(), (what, k, np.argwhere(a[k] != b[k])[:4].tolist())


def single(il, pos, kw, names):
    il.run(*pos, **kw)
    return snapshot(il, names)


def split(il, pos, kw, segments, names, between=None):
    """The segments [(begin, end), ...] one after the other; between(il, begin, end) is called behind each."""
    for b, e in segments:
        il.run_segment(*pos, b, e, **kw)
        if between is not None:
            between(il, b, e)
    return snapshot(il, names)


def _poison_finished(names):
    """between-segments hook: the output rows of chains that are finished get a sentinel (the caller owns the outputs; the workspace is left
    alone), so that a later segment that writes them again -- even the same values -- shows."""
    seen = {}

    def hook(il, b, e):
        torch.cuda.synchronize()
        for c in np.flatnonzero(il.resume[:, 1].cpu().numpy() == 1):
            if int(c) in seen:
                continue
            seen[int(c)] = {k: getattr(il, k)[c].cpu().numpy().copy() for k in names}
            for k in names:
                getattr(il, k)[c] = SENTINEL
    return hook, seen
