"""The NumPy statement of the windowed loops' noise (k_window_noise in csrc/mst_window.h, mst_amd.diffusion.windows.noise_windows) for
tests/test_windows_stochastic_cpu.py and tests/test_gpu_windows_stochastic.py:

    window noise = unfold of the long draw.

Entry j of the buffer [nsteps,N,F,1,W] is unfold(Z_j), Z_j [C,F,1,L] = the engine's Philox normals of C clips of L frames under
(seed, step0 + j) -- oracle/philox.py: element (c, f, l) is component l & 3 of the four normals of counter (l >> 2, f, c, step0 + j).
The draw is in LONG-clip coordinates, so every window that covers a long frame holds the same number for it; window frames at or past
a clip's length are 0.0.  float64: the integer part is exact, the transcendentals are libm's (the kernel's are the hardware's)."""
import numpy as np

from oracle import philox
import window_fixture as wf


def long_draw(C, F, L, seed, step):
    """Z [C,F,1,L] float64."""
    return philox.normal(C, F, L, seed, step)[:, :, None, :]


def window_noise(lengths, W, O, F, L, seed, step0, nsteps):
    """[nsteps,N,F,1,W] float64 over the plan of `lengths` (tests/window_fixture.py: plan, unfold)."""
    win0, starts, clips = wf.plan(lengths, W, O)
    return np.stack([wf.unfold(long_draw(len(lengths), F, L, seed, step0 + j), lengths, win0, starts, clips, W, dtype=np.float64)
                     for j in range(nsteps)])
