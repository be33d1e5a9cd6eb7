"""k_render_bounds / k_render_frames (csrc/mst_render.h) behind `render_motion` against tests/render_fixture.py's float64 restatement.

The bar, per case, on the float image: max |kernel - f64| <= 4 x the float32 restatement's own max |f32 - f64| on the same inputs,
floor 1e-6 (images live in [0, 1], so distances are absolute).  Every distance is printed.  The uint8 image must be exactly
floor(255 f + 0.5) of the kernel's own float image and within 1 level of the float64 restatement's on every pixel; the float32
restatement is held to that cap too.  Every case's three images are computed once and shared."""
import numpy as np
import pytest
import torch

import mst_amd  # noqa: F401
import render_fixture as rf
from mst_amd.utils import plot_script as ps

pytestmark = pytest.mark.gpu
ALL = [(rf.ROOT_HORIZONTAL, 0), (rf.ROOT, 0), (rf.JOINT, 7)]
FEATURES = ["root_horizontal", "root", 7]


def _circle(T, J, seed):
    """A clip whose root circles inside the view, so a long trace stays on the image from its first chunk to its last."""
    w = rf.walk(seed, 1, T, J)
    w[..., [0, 2]] -= w[:, :, :1, [0, 2]]
    k = np.arange(T) * (2 * np.pi / 97.0)
    w[..., 0] += (0.45 * np.cos(k))[None, :, None].astype(np.float32)
    w[..., 2] += (0.45 * np.sin(k) + 0.3 * np.sin(k / 5.3))[None, :, None].astype(np.float32)
    return w


def _behind_and_far(joints, chains, side):
    """The default camera with its w row replaced by one that grows with height, w = 5.5 (y - y0): the head keeps a w near the
    default camera's 10, and y0 is set so that, in frame 0, the second lowest chain joint `b` has w = 0.004, which throws it some
    thousand pixels outside the image, and the lowest, `a`, has w < 0: behind the eye."""
    P, A = ps.default_camera(side, side)
    d = joints[0].astype(np.float64) * 1.3
    d[..., 1] -= d[..., 1].min()
    seen = d[0] - d[0, 0] * np.array([1.0, 0.0, 1.0])
    drawn = sorted({j for c in chains[:5] for j in c}, key=lambda j: seen[j, 1])
    a, b = drawn[0], drawn[1]
    P = P.copy()
    P[3] = (0.0, 5.5, 0.0, 0.004 - 5.5 * seen[b, 1])
    ha, hb = np.append(seen[a], 1.0), np.append(seen[b], 1.0)
    assert P[3] @ ha < 0 < P[3] @ hb < 0.01
    far = np.abs(A @ np.array([P[0] @ hb / (P[3] @ hb), P[1] @ hb / (P[3] @ hb), 1.0])).max()
    assert 20 * side < far < 1e5, far
    return P, A


def _cases():
    chunk = ps.limits()["chunk"]
    c = {}
    c["b1_t1_16"] = dict(joints=rf.walk(11, 1, 1, 22), size=(16, 16), traces=ALL)                      # no trace has two points
    c["b1_t2_37x29"] = dict(joints=rf.walk(12, 1, 2, 21), size=(29, 37), traces=ALL)                   # odd sides, partial tiles, unpacked stores
    c["b3_t9_96"] = dict(joints=rf.walk(13, 3, 9, 20), size=(96, 96), traces=ALL, lengths=[9, 1, 5],
                         palette=np.arange(27).reshape(3, 9) % 4)                                      # many tiles: the culled lists differ by tile
    c["b33_t9_37x29"] = dict(joints=rf.walk(14, 33, 9, 22), size=(29, 37), traces=ALL, lengths=[9 - (b % 4) for b in range(33)])
    c["b1_t3_300"] = dict(joints=rf.walk(15, 1, 3, 22), size=(300, 300), traces=[(rf.ROOT, 0)])
    c["chunk_plus_1_32"] = dict(joints=_circle(chunk + 1, 22, 16), size=(32, 32), traces=[(rf.JOINT, 7), (rf.ROOT_HORIZONTAL, 0)],
                                frames=(chunk - 1, chunk + 1))                                         # a trace of chunk + 1 points: two chunks
    c["joints2_37x29"] = dict(joints=rf.walk(17, 2, 3, 22), joints2=rf.walk(18, 2, 3, 22) + np.float32(0.2), size=(29, 37), traces=ALL)
    c["seven_chains_16"] = dict(joints=rf.walk(19, 1, 2, 22), size=(16, 16), traces=(), chains=rf.chains_of(22) + [[1, 6, 11], [2, 7, 12]])
    j = rf.walk(20, 1, 2, 22)
    c["behind_and_far_32"] = dict(joints=j, size=(32, 32), traces=ALL, camera=_behind_and_far(j, rf.chains_of(22), 32))
    j = rf.walk(21, 1, 2, 22)
    j[..., 0] = np.float32(0.25)
    c["degenerate_quad_16"] = dict(joints=j, size=(16, 16), traces=[(rf.ROOT, 0)])
    return c


_CASES = None
_DONE = {}


def case(name):
    global _CASES
    if _CASES is None:
        _CASES = _cases()
    return _CASES[name]


NAMES = ["b1_t1_16", "b1_t2_37x29", "b3_t9_96", "b33_t9_37x29", "b1_t3_300", "chunk_plus_1_32", "joints2_37x29", "seven_chains_16",
         "behind_and_far_32", "degenerate_quad_16"]


def gpu_render(c, stream=None, **over):
    c = dict(c, **over)
    dev = torch.device("cuda:0")
    J = c["joints"].shape[2]
    kw = dict(lengths=c.get("lengths"), joints2=None if c.get("joints2") is None else torch.from_numpy(c["joints2"]).to(dev),
              palette=c.get("palette"), painting_features=[t[1] if t[0] == rf.JOINT else ("root_horizontal", "root")[t[0]] for t in c["traces"]],
              size=c["size"], camera=c.get("camera"), overlay=c.get("overlay"), frames=c.get("frames"), float_image=True)
    j = torch.from_numpy(c["joints"]).to(dev)
    if stream is None:
        u8, f = ps.render_motion(j, c.get("chains", rf.chains_of(J)), **kw)
    else:
        stream.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(stream):
            u8, f = ps.render_motion(j, c.get("chains", rf.chains_of(J)), **kw)
        stream.synchronize()
    torch.cuda.synchronize()
    return u8.cpu().numpy(), f.cpu().numpy()


def restate(c, dtype):
    H, W = c["size"]
    J = c["joints"].shape[2]
    P, A = c.get("camera") or ps.default_camera(W, H)
    # the reference's order of traces: root_horizontal, root, then the joints
    order = sorted(c["traces"], key=lambda t: t[0])
    return rf.render(c["joints"], c.get("chains", rf.chains_of(J)), c.get("lengths"), dtype=dtype, proj=P, affine=A, W=W, H=H,
                     joints2=c.get("joints2"), palette=c.get("palette"), traces=order, overlay=c.get("overlay"), frames=c.get("frames"))


def done(name):
    if name not in _DONE:
        c = case(name)
        u8, f = gpu_render(c)
        f32, f64 = restate(c, np.float32), restate(c, np.float64)
        own, got = rf.distance(f32, f64), rf.distance(f, f64)
        print(f"{name}: kernel vs f64 {got:.3e}; f32 restatement vs f64 {own:.3e}; bar {rf.bar(own):.3e}; kernel vs f32 restatement "
              f"{rf.distance(f, f32):.3e}")
        _DONE[name] = dict(u8=u8, f=f, f32=f32, f64=f64, own=own, got=got)
    return _DONE[name]


# ------------------------------------------------------------------------------------------ against float64
@pytest.mark.parametrize("name", NAMES)
def test_float_image_against_float64(name):
    r = done(name)
    assert r["f"].dtype == np.float32 and r["f"].shape == r["f64"].shape
    assert np.isfinite(r["f"]).all() and r["f"].min() >= 0.0 and r["f"].max() <= 1.0
    assert r["f64"].min() < 0.9                              # something is drawn
    assert r["got"] <= rf.bar(r["own"]), (name, r["got"], r["own"])


@pytest.mark.parametrize("name", NAMES)
def test_uint8_image(name):
    r = done(name)
    assert r["u8"].dtype == np.uint8
    assert np.array_equal(r["u8"], rf.quantise(r["f"]))      # exactly floor(255 f + 0.5) of the kernel's own float image
    want = rf.quantise(r["f64"]).astype(np.int16)
    worst, worst32 = int(np.abs(r["u8"].astype(np.int16) - want).max()), int(np.abs(rf.quantise(r["f32"]).astype(np.int16) - want).max())
    print(f"{name}: levels from the f64 image: kernel {worst}, f32 restatement {worst32}")
    assert worst32 <= 1                                      # the condition: the rule is continuous
    assert worst <= 1


def test_worst_fraction():
    worst = max((done(n)["got"] / rf.bar(done(n)["own"]), n) for n in NAMES)
    print(f"worst fraction of the bar: {worst[0]:.3f} ({worst[1]})")
    assert worst[0] <= 1.0


def test_cases_are_what_they_claim():
    lim = ps.limits()
    assert case("chunk_plus_1_32")["joints"].shape[1] == lim["chunk"] + 1
    assert len(case("seven_chains_16")["chains"]) == 7 and lim["chains_drawn"] == 5
    c = case("seven_chains_16")
    five = gpu_render(c, chains=c["chains"][:5])
    assert np.array_equal(five[0], done("seven_chains_16")["u8"]) and np.array_equal(five[1], done("seven_chains_16")["f"])
    r = done("degenerate_quad_16")
    assert not np.any(np.all(rf.quantise(r["f64"]) == 191, -1))          # no pixel is the quad's grey
    t1 = done("b1_t1_16")
    assert np.array_equal(t1["f"], gpu_render(case("b1_t1_16"), traces=())[1])   # a clip of one frame has no trace at all
    assert set(case("b3_t9_96")["palette"].reshape(-1).tolist()) == {0, 1, 2, 3}                     # every palette is read


# ------------------------------------------------------------------------------------------ position independence and isolation
def test_a_clips_frames_do_not_depend_on_the_batch_the_stream_or_other_rows():
    c = case("b33_t9_37x29")
    pick, n = 6, 7                                           # lengths[6] = 9 - 2
    assert c["lengths"][pick] == n
    full_u8, full_f = done("b33_t9_37x29")["u8"], done("b33_t9_37x29")["f"]
    want_u8, want_f = full_u8[pick], full_f[pick]
    assert not want_u8[n:].any() and not want_f[n:].any() and want_u8[:n].any()        # exact zeros at and behind the length
    for b, length in enumerate(c["lengths"]):
        assert not full_u8[b, length:].any() and not full_f[b, length:].any()
    alone = gpu_render(c, joints=c["joints"][pick:pick + 1], lengths=[n])
    assert np.array_equal(alone[0][0], want_u8) and np.array_equal(alone[1][0], want_f)
    for place in (0, 32):
        order = [b for b in range(33) if b != pick]
        order.insert(place, pick)
        got = gpu_render(c, joints=c["joints"][order], lengths=[c["lengths"][b] for b in order])
        assert np.array_equal(got[0][place], want_u8) and np.array_equal(got[1][place], want_f), place
    side = gpu_render(c, stream=torch.cuda.Stream())
    assert np.array_equal(side[0], full_u8) and np.array_equal(side[1], full_f)
    poisoned = np.full_like(c["joints"], np.nan)
    poisoned[pick, :n] = c["joints"][pick, :n]
    got = gpu_render(c, joints=poisoned)
    assert np.array_equal(got[0][pick], want_u8) and np.array_equal(got[1][pick], want_f)


@pytest.mark.parametrize("rng", [(0, 1), (8, 9), (3, 6)])
def test_frame_sub_range_equals_the_slice(rng):
    c = case("b3_t9_96")
    got = gpu_render(c, frames=rng)
    assert got[0].shape == (3, rng[1] - rng[0], 96, 96, 3)
    assert np.array_equal(got[0], done("b3_t9_96")["u8"][:, rng[0]:rng[1]]) and np.array_equal(got[1], done("b3_t9_96")["f"][:, rng[0]:rng[1]])


def test_layout_bjct_reads_the_same_clip_in_place():
    c = case("joints2_37x29")
    dev = torch.device("cuda:0")
    j, j2 = (torch.from_numpy(c[k]).to(dev).permute(0, 2, 3, 1).contiguous() for k in ("joints", "joints2"))      # [B, J, 3, T]
    u8 = ps.render_motion(j, rf.chains_of(22), joints2=j2, painting_features=FEATURES, size=c["size"], layout="bjct")
    assert np.array_equal(u8.cpu().numpy(), done("joints2_37x29")["u8"])


# ------------------------------------------------------------------------------------------ the overlay
def test_overlay():
    c = case("joints2_37x29")
    H, W = c["size"]
    g = np.random.default_rng(2)
    ov = np.zeros((2, H, W), np.uint8)
    ov[0, :6] = 255
    ov[1, 10:20, 5:30] = g.integers(1, 255, (10, 25))
    ov[1, 25:, 30:] = 255
    plain_u8, plain_f = done("joints2_37x29")["u8"], done("joints2_37x29")["f"]
    for o in (ov[:1], ov):                                   # [1, H, W] serves every clip, [B, H, W] one each
        u8, f = gpu_render(c, overlay=o)
        f64 = restate(dict(c, overlay=o), np.float64)
        f32 = restate(dict(c, overlay=o), np.float32)
        assert rf.distance(f, f64) <= rf.bar(rf.distance(f32, f64))
        for b in range(2):
            m = o[0 if len(o) == 1 else b]
            assert np.array_equal(f[b][:, m == 0], plain_f[b][:, m == 0]) and np.array_equal(u8[b][:, m == 0], plain_u8[b][:, m == 0])   # bit for bit
            assert not f[b][:, m == 255].any() and not u8[b][:, m == 255].any()                                                         # exact black
            part = (m > 0) & (m < 255)
            if part.any():
                assert (f[b][:, part] <= plain_f[b][:, part]).all() and (f[b][:, part] < plain_f[b][:, part]).any()


# ------------------------------------------------------------------------------------------ the reference's entry points
def test_plot_3d_motion_equals_render_motion_with_its_frame_colors():
    dev = torch.device("cuda:0")
    w = rf.walk(23, 2, 9, 22)
    chains = rf.chains_of(22)
    colors = ps.frame_colors(9, "default", gt_frames=[0, 1, 5])
    assert colors.count("blue") == 3
    kw = dict(figsize=(0.64, 0.8), painting_features="root_horizontal,upper_body,".split(","))      # the demo's mask names: two name no trace
    title = ps.title_overlay("a person walks", 80, 64)
    assert title[:16].any() and not title[16:].any()
    want = ps.render_motion(torch.from_numpy(w).to(dev), chains, palette=colors, painting_features=["root_horizontal"], size=(80, 64),
                            overlay=title).cpu().numpy()
    one = ps.plot_3d_motion(None, chains, w[0], "a person walks", "humanml", gt_frames=[0, 1, 5], **kw)
    assert one.is_cuda and tuple(one.shape) == (9, 80, 64, 3) and np.array_equal(one.cpu().numpy(), want[0])
    flat = ps.plot_3d_motion(None, chains, w[1].reshape(9, -1), "a person walks", "humanml", gt_frames=[0, 1, 5], **kw)      # [T, J * 3], as the reference reshapes
    assert np.array_equal(flat.cpu().numpy(), want[1])
    both = ps.plot_3d_motion(None, chains, torch.from_numpy(w).to(dev), "a person walks", "humanml", gt_frames=[0, 1, 5], **kw)
    assert np.array_equal(both.cpu().numpy(), want)
    # 'gt' is all blue; 'upper_body' draws its orange frames in the upper_body palette
    gt = ps.plot_3d_motion(None, chains, w[0], "", "humanml", vis_mode="gt", **kw)
    assert np.array_equal(gt.cpu().numpy(), ps.render_motion(torch.from_numpy(w[:1]).to(dev), chains, palette="blue",
                                                            painting_features=["root_horizontal"], size=(80, 64))[0].cpu().numpy())
    ub = ps.plot_3d_motion(None, chains, w[0], "", "humanml", vis_mode="upper_body", gt_frames=[2], **kw)
    assert np.array_equal(ub.cpu().numpy(), ps.render_motion(torch.from_numpy(w[:1]).to(dev), chains, palette=[3, 3, 0] + [3] * 6,
                                                            painting_features=["root_horizontal"], size=(80, 64))[0].cpu().numpy())


def test_render_to_file_goes_through_frame_chunks(tmp_path):
    dev = torch.device("cuda:0")
    w = torch.from_numpy(rf.walk(24, 1, 9, 22)).to(dev)
    path = ps.render_to_file(tmp_path / "clip.npy", w, rf.chains_of(22), chunk=4, painting_features=["root"], size=32)
    assert np.array_equal(np.load(path), ps.render_motion(w, rf.chains_of(22), painting_features=["root"], size=32)[0].cpu().numpy())
