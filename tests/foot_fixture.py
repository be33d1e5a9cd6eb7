"""numpy restatement of the reference's foot-skate cleanup, and the seeded clips the tests run it on.

What is restated (data_loaders/humanml/common/bvh_utils.py): `remove_fs` :1685-1809 -- floor shift, contact runs replaced by their mean,
blend of the frames around a run -- with `get_foot_contact_by_vel_acc` :1591-1639, `get_foot_contact_by_vel3` :1642-1682 and the
forward-backward `Butterworth` :1872-1916.  `ref_height` is left out: no caller passes it.

`dtype` switches the precision.  np.float32 is the reference's own: fp32 arrays, Python-float (double) blend weights rounded to fp32 where
numpy rounds them, the filter in float64 and its result stored as fp32; in this form the functions are bit-equal to the reference on every
golden case (tests/test_foot_cleanup_cpu.py).  np.float64 evaluates the same formulas from the same fp32 inputs without any fp32 rounding:
the distance between the two is the reference's own error, and `bar()` of it is what the kernel is held to.

vel_acc at two frames: the reference builds an EMPTY contact array there and raises IndexError on its first read; here (and in the kernel)
a two-frame clip simply has no contact in that mode, the same "pad one zero at both ends" with nothing in between.

A flipped contact bit changes a whole run, so no comparison may sit near its threshold.  `make_clip` builds clips for that: every value a
detector compares is at least MARGIN (10 %) of the threshold away from it -- foot speeds against every vel3 threshold in THR3, |vy|
against 0.003, and, for the sign tests and the window, |vy|, |acc| and heights against their own thresholds.  `margins()` measures it."""
import numpy as np

import mst_amd.synthetic as syn

FLOOR = 1e-6
THR3 = (0.02, 0.05)          # the vel3 thresholds the tests use (demo_style_transfer.py:214, :312)
VTHR = 0.003                 # remove_fs's vel_acc threshold
WINDOW, HTHR = 3, 0.006      # use_window
MARGIN = 0.10
NAMES22 = ["Hips", "mixamorig:LeftUpLeg", "mixamorig:RightUpLeg", "Spine", "LeftLeg", "RightLeg", "Spine1", "LeftFoot", "RightFoot",
           "Spine2", "LeftToeBase", "RightToeBase", "Neck", "LeftShoulder", "RightShoulder", "Head", "LeftArm", "RightArm",
           "LeftForeArm", "RightForeArm", "LeftHand", "RightHand"]
EE_NAMES = ["RightToeBase", "LeftToeBase", "LeftFoot", "RightFoot"]       # get_ee_id_by_names's default order
FID22 = (11, 10, 7, 8)


def f64(a):
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    return np.asarray(a, dtype=np.float64)


def rel(a, b):
    a, b = f64(a), f64(b)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def bar(ref_deviation):
    """4 x the reference's own fp32 deviation, floor 1e-6: the rule of tests/glue_fixture.py."""
    return max(4.0 * float(ref_deviation), FLOOR)


# ------------------------------------------------------------------------------------------ the restatement
def butterworth_coefficients(cutoff, dt=1 / 20):
    rate = 1 / dt
    pi = 3.14159265358979
    wc = np.tan(cutoff * pi / rate)
    k1 = 1.414213562 * wc
    k2 = wc * wc
    a = k2 / (1 + k1 + k2)
    b = 2 * a
    k3 = b / k2
    return a, b, a, -2 * a + k3, 1 - (2 * a) - k3


def butterworth(x, cutoff):
    """x [n, ...]: every column along axis 0 filtered as the reference filters one (float64 recursion, result in x's dtype); the last
    frame keeps its value.  Vectorised over the columns, sequential over the frames: each column sees the reference's operations."""
    n = x.shape[0]
    a, b, c, d, e = butterworth_coefficients(cutoff)
    cols = x.reshape(n, -1)
    X = np.concatenate([cols[:1], cols[:1], cols, cols[-1:]], axis=0).astype(np.float64)          # Dat2: n + 3 rows
    Y = np.zeros_like(X)
    Y[0] = Y[1] = cols[0]
    for s in range(2, n + 1):
        Y[s] = a * X[s] + b * X[s - 1] + c * X[s - 2] + d * Y[s - 1] + e * Y[s - 2]
    Y[n + 2] = Y[n + 1] = Y[n]
    Z = np.zeros((n + 1, cols.shape[1]))
    Z[n - 1], Z[n] = Y[n + 1], Y[n + 2]
    for i in range(n - 2, -1, -1):
        Z[i] = a * Y[i + 2] + b * Y[i + 3] + c * Y[i + 4] + d * Z[i + 1] + e * Z[i + 2]
    out = cols.copy()
    out[:n - 1] = Z[:n - 1]
    return out.reshape(x.shape)


def contacts_vel3(ref, fid, thr):
    """-> contacts [n, 4] int32, speeds [n-1, 4]."""
    pos = ref[:, list(fid), :]
    vel = pos[1:] - pos[:-1]
    speed = np.linalg.norm(vel, ord=2, axis=-1)
    hit = speed < ref.dtype.type(thr)
    return np.concatenate([hit, np.zeros((1, 4), bool)], axis=0).astype(np.int32), speed


def contacts_vel_acc(ref, fid, thr=VTHR, use_window=False):
    """-> contacts [n, 4] int32, y-velocities [n-1, 4]."""
    n = ref.shape[0]
    y = ref[:, list(fid), 1]
    v = y[1:] - y[:-1]
    acc = v[1:] - v[:-1]
    t = ref.dtype.type
    hit = ((np.abs(v[:-1]) < t(thr)) & (acc > 0)) | ((v[:-1] < 0) & (v[1:] > 0))
    raw = np.zeros((n, 4), np.int32)
    raw[1:n - 1] = hit
    new = raw.copy()
    if use_window:
        for i in range(4):
            for frame in range(n):
                if raw[frame, i] == 1:
                    start, end = max(frame - WINDOW, 0), min(frame + WINDOW + 1, n)
                    new[start:end, i] = np.abs(y[start:end, i] - y[frame, i]) < t(HTHR)
    return new, v


def remove_fs(glb, ref, fid, interp_length=5, force_on_floor=False, use_window=False, use_vel3=False, use_butterworth=False,
              vel3_thr=0.01, after_butterworth=False, dtype=np.float32):
    """One clip [n, J, 3] -> (cleaned clip, foot_vels, contacts), all in `dtype` (contacts int32)."""
    glb = np.array(glb, dtype=dtype)
    ref = glb.copy() if ref is None else np.array(ref, dtype=dtype)
    n = len(glb)
    if n < 2:
        raise IndexError("a one-frame clip has no velocity")
    if use_butterworth:
        glb = butterworth(glb, 3)
    glb[:, :, 1] -= glb[..., 1].min()
    if use_vel3:
        contacts, vels = contacts_vel3(ref, fid, vel3_thr)
    else:
        contacts, vels = contacts_vel_acc(ref, fid, VTHR, use_window)

    def alpha(t):
        return 2.0 * t * t * t - 3.0 * t * t + 1

    def lerp(a, l, r):
        return (1 - a) * l + a * r
    L = interp_length
    for i, fidx in enumerate(fid):
        fixed = contacts[:, i]
        s = 0
        while s < n:
            while s < n and fixed[s] == 0:
                s += 1
            if s >= n:
                break
            t = s
            avg = glb[t, fidx].copy()
            while t + 1 < n and fixed[t + 1] == 1:
                t += 1
                avg += glb[t, fidx]
            avg /= (t - s + 1)
            if force_on_floor:
                avg[1] = 0.0
            glb[s:t + 1, fidx] = avg
            s = t + 1
        for s in range(n):
            if fixed[s] == 1:
                continue
            l = next((s - k - 1 for k in range(L) if s - k - 1 >= 0 and fixed[s - k - 1]), None)
            r = next((s + k + 1 for k in range(L) if s + k + 1 < n and fixed[s + k + 1]), None)
            if l is None and r is None:
                continue
            if l is not None and r is not None:
                litp = lerp(alpha(1.0 * (s - l + 1) / (L + 1)), glb[s, fidx], glb[l, fidx])
                ritp = lerp(alpha(1.0 * (r - s + 1) / (L + 1)), glb[s, fidx], glb[r, fidx])
                glb[s, fidx] = lerp(alpha(1.0 * (s - l + 1) / (r - l + 1)), ritp, litp)
            elif l is not None:
                glb[s, fidx] = lerp(alpha(1.0 * (s - l + 1) / (L + 1)), glb[s, fidx], glb[l, fidx])
            else:
                glb[s, fidx] = lerp(alpha(1.0 * (r - s + 1) / (L + 1)), glb[s, fidx], glb[r, fidx])
    if after_butterworth:
        glb = butterworth(glb, 2.5)
    return glb, vels, contacts


def remove_fs_batch(glb, ref, fid, lengths=None, dtype=np.float32, **kw):
    """glb [B, T, J, 3], ref None or [B or 1, T, J, 3] -> (clips [B, T, J, 3], foot_vels [B, T-1, 4], contacts [B, T, 4]); every stage
    sees frames 0 .. len-1, later frames pass through and their contacts and velocities are zero."""
    B, T = glb.shape[:2]
    out = np.array(glb, dtype=dtype)
    vels, contacts = np.zeros((B, T - 1, 4), dtype), np.zeros((B, T, 4), np.int32)
    for b in range(B):
        n = T if lengths is None else int(lengths[b])
        r = None if ref is None else ref[b if len(ref) > 1 else 0][:n]
        out[b, :n], vels[b, :n - 1], contacts[b, :n] = remove_fs(glb[b, :n], r, fid, dtype=dtype, **kw)
    return out, vels, contacts


def demo_passes(glb, ref, fid, lengths=None, dtype=np.float32, passes=2, vel3_thr=0.05):
    """sample/demo_style_transfer.py:312-313: pass 1 against the content motion, later passes against the clip itself."""
    kw = dict(force_on_floor=True, after_butterworth=True, use_vel3=True, vel3_thr=vel3_thr)
    for k in range(passes):
        glb = remove_fs_batch(glb, ref if k == 0 else None, fid, lengths, dtype, **kw)[0]
    return glb


# ------------------------------------------------------------------------------------------ clips built for the margin
def random_stance(seed, tag, T):
    """[T-1, 4] bool: stance and swing phases of 1 .. 12 frames, per foot."""
    st = np.zeros((T - 1, 4), bool)
    for i in range(4):
        u = syn.uniform01(seed, f"{tag}/phase{i}", 2 * T + 2)
        t, on, k = 0, u[0] < 0.5, 1
        while t < T - 1:
            run = 1 + int(u[k] * 12)
            st[t:t + run, i] = on
            t, on, k = t + run, not on, k + 1
    return st


def sparse_stance(seed, tag, T, phases=2):
    """[T-1, 4] bool: `phases` stance phases of 12 .. 30 frames per foot, swing elsewhere (few transitions: the demo's second pass
    detects contacts on the FILTERED output of the first, whose speeds near a transition nobody plants)."""
    st = np.zeros((T - 1, 4), bool)
    for i in range(4):
        u = syn.uniform01(seed, f"{tag}/sparse{i}", 2 * phases)
        for k in range(phases):
            seg = (T - 1) // phases
            run = 12 + int(u[2 * k] * 18)
            start = k * seg + int(u[2 * k + 1] * max(seg - run - 2, 1)) + 1
            st[start:start + run, i] = True
    return st


def golden_cases(T):
    """The detector x flag combinations tests/golden/fs.npz holds for a clip of T frames (J = 22): the full cross up to T = 65, eight
    combinations that still show every value of every switch at T = 196.  `ref` says whether contacts are detected on the clip itself or
    on a second clip.  vel_acc needs three frames (at two the reference raises IndexError)."""
    dets = [("vel3_0.02", dict(use_vel3=True, vel3_thr=0.02)), ("vel3_0.05", dict(use_vel3=True, vel3_thr=0.05)),
            ("acc", dict(use_vel3=False, use_window=False)), ("acc_win", dict(use_vel3=False, use_window=True))]
    filts = [("off", dict()), ("after", dict(after_butterworth=True)), ("both", dict(use_butterworth=True, after_butterworth=True))]
    cases = []
    for d, (dn, dk) in enumerate(dets):
        if T < 3 and not dk["use_vel3"]:
            continue
        for force in (False, True):
            for f, (fn, fk) in enumerate(filts):
                if T > 65 and (d + 2 * force + f) % 3 != 0:
                    continue
                ref = "other" if (d + force + f) % 2 else "self"
                cases.append(dict(tag=f"{dn}|{'floor' if force else 'free'}|{fn}|{ref}", det=dn, ref=ref,
                                  kw=dict(force_on_floor=force, **dk, **fk)))
    return cases


GOLDEN_T = (2, 3, 7, 65, 196)
GOLDEN_EVERY = {2: 1, 3: 1, 7: 1, 65: 8, 196: 16}           # fs.npz keeps every k-th frame of the joints that are not feet
DEMO_T, DEMO_LEN = 196, 180


def golden_inputs(seed, T):
    """(clip, other clip) of the golden cases at T frames."""
    return make_clip(seed, f"fs/T{T}/glb", T, 22, FID22), make_clip(seed, f"fs/T{T}/ref", T, 22, FID22)


def demo_inputs(seed, variant):
    """(sample [1, 263, 1, 196], mean, std, content joints [196, 22, 3]) of the demo composition; `variant` is the stream the generator
    settled on (the first whose SECOND pass also keeps every speed 10 % away from the threshold), stored in fs.npz."""
    tag = f"fs/demo{variant}"
    clip = make_clip(seed, f"{tag}/glb", DEMO_T, 22, FID22, sparse_stance(seed, f"{tag}/glb", DEMO_T))
    ref = make_clip(seed, f"{tag}/ref", DEMO_T, 22, FID22, sparse_stance(seed, f"{tag}/ref", DEMO_T))
    sample, mean, std = sample_from_joints(clip, seed, tag)
    return sample[None], mean, std, ref


def planted_stance(pattern, n, L):
    """[n-1] bool contact bits of frames 0 .. n-2 (frame n-1 is never in contact) for a named pattern; L = interp_length."""
    m = n - 1
    if pattern == "none":
        return np.zeros(m, bool)
    if pattern == "all":
        return np.ones(m, bool)
    if pattern == "from0":                                   # a run from frame 0, then nothing
        return np.arange(m) < max(1, m // 3)
    if pattern == "to_end":                                  # a run ending at n-2
        return np.arange(m) >= m - max(1, m // 3)
    if pattern == "single":                                  # one-frame runs, 2 L + 2 apart
        return np.arange(m) % (2 * L + 2) == L
    if pattern == "gaps":
        # start gap L-1 | run | L | run | L+1 | run | 2L | run | 2L+1 | run, repeated; the end is cut so that a run stops L-1
        # frames before the last frame (which, never in contact, makes the end gap L frames at most)
        unit = [0] * (L - 1) + [1, 1] + [0] * L + [1] + [0] * (L + 1) + [1, 1, 1] + [0] * (2 * L) + [1] + [0] * (2 * L + 1) + [1, 1]
        seq = (unit * (m // len(unit) + 1))[:m]
        seq = np.array(seq, bool)
        tail = max(L - 2, 0)
        if m > tail + 2:
            seq[m - tail:] = False
            seq[m - tail - 2:m - tail] = True
        return seq
    raise ValueError(pattern)


def _violation(vy):
    """First interval whose planted vy breaks a vel_acc / window margin (with slack for the fp32 rounding of the positions), or -1."""
    slack = 1.4
    bad = np.zeros(len(vy), bool)
    bad |= np.abs(np.abs(vy) - VTHR) < slack * MARGIN * VTHR
    bad |= np.abs(vy) < slack * MARGIN * VTHR
    bad[1:] |= np.abs(vy[1:] - vy[:-1]) < slack * MARGIN * VTHR
    c = np.concatenate([[0.0], np.cumsum(vy)])
    for w in range(1, WINDOW + 1):                           # heights |y[k+w] - y[k]|
        near = np.abs(np.abs(c[w:] - c[:-w]) - HTHR) < slack * MARGIN * HTHR
        bad[:len(near)] |= near
    idx = np.flatnonzero(bad)
    return int(idx[0]) if len(idx) else -1


def make_clip(seed, tag, T, J, fid, stance=None):
    """[T, J, 3] float32.  stance [T-1, 4] bool (default: random phases): under vel3 with any threshold of THR3 the contacts of frames
    0 .. T-2 ARE these bits -- a stance interval moves a foot by <= 0.005, a swing interval by >= 0.11.  The vertical velocity of every
    foot is drawn away from the vel_acc thresholds and redrawn, one interval at a time, until every margin holds."""
    if stance is None:
        stance = random_stance(seed, tag, T)
    body = 0.9 + 0.4 * syn.normal(seed, f"{tag}/body", (T, J, 3)).astype(np.float64)
    walk = np.cumsum(0.02 * syn.normal(seed, f"{tag}/walk", (T, J, 3)).astype(np.float64), axis=0)
    clip = body * 0.1 + walk + 0.9
    for i, f in enumerate(fid):
        st = stance[:, i]
        m = T - 1
        u = syn.uniform01(seed, f"{tag}/foot{i}", 5 * m).reshape(5, m)
        speed = np.where(st, 0.004 * u[0], 0.11 + 0.19 * u[0])
        # one heading per phase (a swing carries the foot somewhere; a new heading every frame would be noise the filter removes),
        # a little jitter per interval
        phase = np.concatenate([[0], np.cumsum(st[1:] != st[:-1])])
        ang = 2 * np.pi * syn.uniform01(seed, f"{tag}/heading{i}", m)[phase] + 0.3 * (u[1] - 0.5)

        def draw(st_t, u_mag, u_kind, u_sign):
            small = st_t or u_kind < 0.5
            mag = 0.0004 + 0.0021 * u_mag if small else 0.0036 + 0.0264 * u_mag
            return mag if u_sign < 0.5 else -mag
        vy = np.array([draw(st[t], u[2, t], u[3, t], u[4, t]) for t in range(m)])
        fix = syn.uniform01(seed, f"{tag}/fix{i}", 3 * 40 * max(m, 8)).reshape(-1, 3)
        k = 0
        while True:
            t = _violation(vy)
            if t < 0:
                break
            vy[t] = draw(st[t], *fix[k])
            k += 1
        vel = np.stack([speed * np.cos(ang), vy, speed * np.sin(ang)], axis=1)
        start = 0.5 * syn.normal(seed, f"{tag}/start{i}", (3,)).astype(np.float64) + np.array([0.0, 0.3, 0.0])
        clip[:, f] = start + np.concatenate([np.zeros((1, 3)), np.cumsum(vel, axis=0)])
    return clip.astype(np.float32)


def margins(clip, fid, thr3=THR3):
    """Smallest distance of any compared value from its threshold, as a fraction of the threshold, over every prefix length of `clip`
    (the conditions are local in time): -> {"vel3": .., "vel_acc": .., "window": ..}; all must be >= MARGIN."""
    c = f64(clip)[:, list(fid)]
    speed = np.linalg.norm(c[1:] - c[:-1], axis=-1)
    out = {"vel3": min(float(np.abs(speed - t).min() / t) for t in thr3)}
    vy = c[1:, :, 1] - c[:-1, :, 1]
    acc = vy[1:] - vy[:-1]
    va = min(float(np.abs(np.abs(vy) - VTHR).min()), float(np.abs(vy).min()))
    if len(acc):
        va = min(va, float(np.abs(acc).min()))
    out["vel_acc"] = va / VTHR
    y = c[:, :, 1]
    w = [float(np.abs(np.abs(y[k:] - y[:-k]) - HTHR).min()) for k in range(1, WINDOW + 1) if k < len(y)]
    out["window"] = min(w) / HTHR
    return out


def sample_from_joints(clip, seed, tag, feats=263):
    """A normalised hml_vec sample [feats, 1, T] (with its mean and std) that `recover_from_ric` turns back into `clip` [T, J, 3] up to fp32
    rounding: zero yaw and root velocity (features 0-2, so that the root stays over the origin and every joint is its local position),
    root height in feature 3, joint j >= 1 in features 4 + 3 (j - 1) ..; the features behind them, which recovery ignores, are noise.
    The root joint's x and z are lost (the root of a recovered clip is at x = z = 0)."""
    T, J = clip.shape[:2]
    mean = (syn.normal(seed, f"{tag}/mean", (feats,)) * 0.3).astype(np.float32)
    std = syn.uniform(seed, f"{tag}/std", (feats,), 0.2, 1.5).astype(np.float32)
    mean[:3] = 0.0
    want = syn.normal(seed, f"{tag}/rest", (T, feats)).astype(np.float64)
    want[:, :3] = 0.0
    want[:, 3] = clip[:, 0, 1]
    want[:, 4:4 + 3 * (J - 1)] = f64(clip)[:, 1:].reshape(T, -1)
    x = (want - f64(mean)) / f64(std)
    x[:, :3] = 0.0
    return np.ascontiguousarray(x.T[:, None, :]).astype(np.float32), mean, std
