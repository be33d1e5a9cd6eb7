"""The NumPy statement of the window glue (csrc/mst_window.h, mst_amd/diffusion/windows.py) for tests/test_windows_cpu.py and
tests/test_gpu_windows.py, in float32 and in float64: the oracle package stays as it is, so this lives here.

Plan.  Clip lengths len[c] (1 <= len[c] <= L), window W, overlap O (1 <= O <= W - 1; a one-frame window cannot overlap, so W == 1
takes O == 0 alone), stride S = W - O.  len <= W: one window at start 0, frames >= len are zero padding.  Otherwise starts 0, S, 2S, ...
while start + W < len, then one last window at len - W, dropped if it coincides with the one before it.  Stored form: windows of clip
c are clip_win0[c] .. clip_win0[c + 1] - 1, window n starts at win_start[n], win_clip[n] is its clip.

Weight.  h(i) = min(i + 1, W - i) at local frame i.

Stitch, in place on [N,F,1,W], for long frame f < len[c] of clip c, K = the windows covering f in ascending order:
    |K| == 1                              not touched
    all of K hold the same bits           kept
    otherwise                             v = (sum_K h x) / (sum_K h), every product and every sum rounded to `dtype` on its own, in
                                          ascending window order; v stored into every window of K
Fold.  long[c, :, 0, f] = the single covering value, or v (or the common bits), for f < len[c]; exactly 0.0 from len[c] on.
Unfold.  The gather the other way; window frames at or past len[c] get 0.0."""
import numpy as np


def plan(lengths, W, O):
    """(clip_win0, win_start, win_clip) int32 -- written out independently of mst_amd.diffusion.windows.plan_windows."""
    assert W >= 1 and (1 <= O <= W - 1 or (W == 1 and O == 0))
    S = W - O
    win0, starts, clips = [0], [], []
    for c, n in enumerate(lengths):
        n = int(n)
        assert n >= 1
        own = []
        if n <= W:
            own.append(0)
        else:
            s = 0
            while s + W < n:
                own.append(s)
                s += S
            if not own or own[-1] != n - W:
                own.append(n - W)
        starts.extend(own)
        clips.extend([c] * len(own))
        win0.append(len(starts))
    return np.asarray(win0, np.int32), np.asarray(starts, np.int32), np.asarray(clips, np.int32)


def weight(W):
    i = np.arange(W)
    return np.minimum(i + 1, W - i)


def covering(lengths, win0, starts, W, c, f):
    """Windows of clip c that cover long frame f, ascending."""
    return [n for n in range(int(win0[c]), int(win0[c + 1])) if starts[n] <= f < starts[n] + W and f < lengths[c]]


def unfold(long, lengths, win0, starts, clips, W, dtype=np.float32):
    long = np.asarray(long, dtype=dtype)
    C, F, _, L = long.shape
    out = np.zeros((len(starts), F, 1, W), dtype=dtype)
    for n, (s, c) in enumerate(zip(starts, clips)):
        k = max(0, min(W, int(lengths[c]) - int(s)))
        out[n, :, 0, :k] = long[c, :, 0, s:s + k]
    return out


def stitch(win, lengths, win0, starts, clips, W, L, dtype=np.float32):
    """(stitched windows, folded long) in `dtype`; the input is not modified.  The same-bits rule is judged on the values AS GIVEN (cast
    to float32 and compared as bit patterns: NaNs with equal payloads agree, +0.0 and -0.0 do not), for both dtypes alike."""
    given = np.ascontiguousarray(np.asarray(win, dtype=np.float32))
    bits = given.view(np.uint32)
    out = given.astype(dtype)
    N, F = out.shape[:2]
    C = len(lengths)
    long = np.zeros((C, F, 1, L), dtype=dtype)
    h = weight(W)
    for c in range(C):
        n0, n1 = int(win0[c]), int(win0[c + 1])
        for f in range(int(lengths[c])):
            K = [n for n in range(n0, n1) if starts[n] <= f < starts[n] + W]
            assert K, (c, f)
            i0 = f - starts[K[0]]
            if len(K) == 1:
                long[c, :, 0, f] = out[K[0], :, 0, i0]
                continue
            same = np.ones(F, dtype=bool)
            num = np.zeros(F, dtype=dtype)
            den = 0
            for n in K:
                i = f - starts[n]
                same &= bits[n, :, 0, i] == bits[K[0], :, 0, i0]
                num = (num + (dtype(h[i]) * out[n, :, 0, i]).astype(dtype)).astype(dtype)
                den += int(h[i])
            with np.errstate(invalid="ignore"):
                v = (num / dtype(den)).astype(dtype)
            v = np.where(same, out[K[0], :, 0, i0], v)
            for n in K:
                out[n, :, 0, f - starts[n]] = v
            long[c, :, 0, f] = v
    return out, long


def fold(win, lengths, win0, starts, clips, W, L, dtype=np.float32):
    return stitch(win, lengths, win0, starts, clips, W, L, dtype)[1]


FLOOR = 1e-6


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def bar(ref_deviation):
    """4 x the float32 statement's own distance from the float64 one, floor 1e-6: the rule of tests/glue_fixture.py."""
    return max(4.0 * float(ref_deviation), FLOOR)
