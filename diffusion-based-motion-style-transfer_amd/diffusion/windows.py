"""Clips of any length through a sampler whose clips are at most `engine.MAX_FRAMES` long: overlapping windows, stitched every step.

No reference counterpart -- the reference cuts the content clip at max_frames (sample/demo_style_transfer.py:37-38, :184).  The
feature rows are frame-local (the root enters as velocities, everything else is relative to the root), so rows [s, s + W) of a long
clip are the rows of the sub-clip: a long clip [C,F,1,L] is cut into windows [N,F,1,W] of the model's own length, all windows of all
clips are sampled as one batch, and after every step the frames two or more windows share are replaced, in all of them, by one
weighted mean (MultiDiffusion / DoubleTake-style synchronisation).  The arithmetic is csrc/mst_window.h; this is the plan and the
plumbing.  `GaussianDiffusion.ddim_sample_loop_windows` is the deterministic loop, `sample_loop_windows` / `p_sample_loop_windows` the
general one: ancestral, stochastic DDIM and guided.  Their noise is drawn in long-clip coordinates (`noise_windows`), so windows that
share a long frame receive the same number for it and the stitch stays exact bookkeeping.

The plan rule (`plan_windows`), stride S = W - O:
  len <= W    one window at start 0; its frames >= len are zero padding, as the demo pads;
  otherwise   starts 0, S, 2S, ... while start + W < len, then one last window at len - W (dropped if it coincides with the one
              before it): every window is full, starts ascend strictly, every frame < len is covered.
The overlap is 1 <= O <= W - 1; a one-frame window cannot overlap, so W == 1 takes O == 0 alone."""
import ctypes as C

import numpy as np
import torch

from .. import _native as N


def plan_windows(lengths, window, overlap):
    """(clip_win0 [C + 1], win_start [N], win_clip [N]) int32, host only: windows clip_win0[c] .. clip_win0[c + 1] - 1 are clip c's."""
    W, O = int(window), int(overlap)
    if W < 1:
        raise ValueError(f"window {W} must be at least 1 frame")
    if not (1 <= O <= W - 1 or (W == 1 and O == 0)):
        raise ValueError(f"overlap {O} outside 1..window - 1 = {W - 1} (a one-frame window takes overlap 0)")
    S = W - O
    win0, starts, clips = [0], [], []
    for c, n in enumerate(int(v) for v in np.asarray(lengths).reshape(-1)):
        if n < 1:
            raise ValueError(f"clip {c}: length {n} must be at least 1")
        if n <= W:
            own = [0]
        else:
            own = list(range(0, n - W, S))          # start + W < len
            if own[-1] != n - W:
                own.append(n - W)
        starts += own
        clips += [c] * len(own)
        win0.append(len(starts))
    return np.asarray(win0, np.int32), np.asarray(starts, np.int32), np.asarray(clips, np.int32)


def window_count(length, window, overlap):
    """Windows of one clip under the plan rule: 1, or ceil((len - W) / S) + 1."""
    n, W, S = int(length), int(window), int(window) - int(overlap)
    return 1 if n <= W else -(-(n - W) // S) + 1


class WindowPlan:
    """The cut of C long clips into N windows, on the device (mst_window_plan).  lengths: the clips' frame counts; long_frames: L of the
    long tensors [C,F,1,L] (default: the longest clip).  Host arrays: .lengths, .clip_win0, .win_start, .win_clip, .win_lengths
    (min(len - start, W) per window); .n_clips, .n_windows, .window, .overlap, .long_frames."""

    def __init__(self, lengths, window, overlap, device, long_frames=None):
        self.device = torch.device(device)
        self.lengths = np.ascontiguousarray(np.asarray(lengths.detach().cpu() if isinstance(lengths, torch.Tensor) else lengths,
                                                       dtype=np.int64).reshape(-1).astype(np.int32))
        if self.lengths.size < 1:
            raise ValueError("WindowPlan: no clips")
        self.window, self.overlap = int(window), int(overlap)
        self.clip_win0, self.win_start, self.win_clip = plan_windows(self.lengths, self.window, self.overlap)
        self.n_clips, self.n_windows = int(self.lengths.size), int(self.win_start.size)
        self.long_frames = int(self.lengths.max()) if long_frames is None else int(long_frames)
        self.win_lengths = np.minimum(self.lengths[self.win_clip] - self.win_start, self.window).astype(np.int32)
        self.handle = _create(self.lengths, self.clip_win0, self.win_start, self.window, self.long_frames, self.device.index or 0)
        self._win_clip_dev = None

    def win_clip_tensor(self):
        """win_clip as an int64 tensor on the plan's device (gathers of per-clip conditioning), uploaded once."""
        if self._win_clip_dev is None:
            self._win_clip_dev = torch.from_numpy(self.win_clip.astype(np.int64)).to(self.device)
        return self._win_clip_dev

    def __del__(self):
        h = getattr(self, "handle", None)
        if h and N is not None and N._lib is not None:      # None during interpreter shutdown
            N._lib.mst_window_plan_destroy(h)
            self.handle = None


def _i32(a):
    a = np.ascontiguousarray(np.asarray(a, dtype=np.int32))
    return a, a.ctypes.data_as(C.POINTER(C.c_int32))


def _create(lengths, clip_win0, win_start, window, long_frames, device_index, n_clips=None, n_windows=None):
    """mst_window_plan_create on host arrays as they are (the library validates them and names what it refuses) -> handle."""
    l, lp = _i32(lengths)
    w0, w0p = _i32(clip_win0)
    st, stp = _i32(win_start)
    h = C.c_void_p()
    N.check(N.lib().mst_window_plan_create(lp, w0p, stp, int(l.size if n_clips is None else n_clips),
                                           int(st.size if n_windows is None else n_windows), int(window), int(long_frames),
                                           int(device_index), C.byref(h)))
    return h


def _check(t, shape, what, plan):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.device == plan.device and t.dtype == torch.float32 and t.is_contiguous()):
        raise ValueError(f"{what}: a contiguous float32 tensor on {plan.device}")
    if t.dim() != 4 or t.shape[0] != shape[0] or t.shape[2] != 1 or t.shape[3] != shape[1]:
        raise ValueError(f"{what}: shape {tuple(t.shape)} is not [{shape[0]}, F, 1, {shape[1]}]")


def unfold(long, plan):
    """long [C,F,1,L] -> windows [N,F,1,W]; window frames at or past a clip's length are 0.0."""
    _check(long, (plan.n_clips, plan.long_frames), "unfold: long", plan)
    F = long.shape[1]
    win = torch.empty((plan.n_windows, F, 1, plan.window), dtype=torch.float32, device=plan.device)
    N.check(N.lib().mst_window_unfold(plan.handle, N.ptr(long), F, N.ptr(win), N.stream_ptr(plan.device)))
    return win


def stitch_(windows, plan, long_out=None):
    """In place on windows [N,F,1,W]: every frame two or more windows share becomes one weighted mean in all of them (singly covered
    frames and frames whose covering windows agree bit for bit are not touched).  long_out: a [C,F,1,L] tensor that also receives
    the fold.  Returns windows."""
    _check(windows, (plan.n_windows, plan.window), "stitch_: windows", plan)
    if long_out is not None:
        _check(long_out, (plan.n_clips, plan.long_frames), "stitch_: long_out", plan)
        if long_out.shape[1] != windows.shape[1]:
            raise ValueError(f"stitch_: long_out has {long_out.shape[1]} features, the windows {windows.shape[1]}")
    N.check(N.lib().mst_window_stitch(plan.handle, N.ptr(windows), windows.shape[1], N.ptr(long_out), N.stream_ptr(plan.device)))
    return windows


def fold(windows, plan):
    """windows [N,F,1,W] -> long [C,F,1,L]: the single covering value, or the stitch's weighted mean, below a clip's length; exactly
    0.0 from there on.  `windows` is left as it is (the stitch runs on a copy)."""
    long = torch.empty((plan.n_clips, windows.shape[1], 1, plan.long_frames), dtype=torch.float32, device=plan.device)
    stitch_(windows.clone(), plan, long_out=long)
    return long


def noise_windows(plan, feats, seed, step0, nsteps):
    """The noise of `nsteps` stochastic steps, drawn in long-clip coordinates (mst_window_noise) -> [nsteps, N, F, 1, W], the buffer a
    windowed loop reads.  Entry j is unfold(Z_j), Z_j [C,F,1,L] = the engine's philox_normal(C, L, seed, step0 + j): every window that
    covers a long frame holds the same bits for it; window frames at or past a clip's length are 0.0."""
    out = torch.empty((int(nsteps), plan.n_windows, int(feats), 1, plan.window), dtype=torch.float32, device=plan.device)
    N.check(N.lib().mst_window_noise(plan.handle, int(feats), int(seed), int(step0), int(nsteps), N.ptr(out), N.stream_ptr(plan.device)))
    return out
