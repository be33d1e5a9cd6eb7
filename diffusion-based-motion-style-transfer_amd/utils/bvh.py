"""BVH motion files in and out: the counterparts of `read_bvh` (data_loaders/humanml/common/bvh_utils.py:84-295), `save_bvh` / `save_joint`
(:499-614, :735-789) and the `Anim` they exchange (:29-81).  The reference parses, converts and formats clip by clip in Python loops; here
the host does text only -- `parse_bvh` turns a file into one float32 array of channel values, `format_bvh` turns one back into text -- and
everything between is one launch for a batch of clips (csrc/mst_bvh.h): `decode_channels` (Euler degrees -> quaternions, the sign
continuity of `remove_quat_discontinuities`, sub-sampling, `quat_fk`, joint selection) and `quats_to_channels` (`q2eul`, degrees, the
writer's joint order).  `parse_bvh` and `format_bvh` need no GPU; nothing else here has a CPU path.

A fractional `downsample_rate` (the reference's slerp up-sampling) is `read_bvh_resampled`, over utils/pose_track.py's
`resample_tracks`; `read_bvh`, `load_bvh` and `decode_channels` take whole rates only.  Not covered: the nine-channel files,
`read_bvh_raw_motion` / `save_bvh_raw_motion`, and an `Anim` whose offsets include End Sites while its quaternions do not.

Stated deviations from the reference's writer: it permutes the quaternions into its depth-first joint order but reads the positions (with
`positions=True`) and drops End Sites (an `Anim` read with `end_sites=True`) by unpermuted index, so its files are wrong unless the joints
already are in depth-first order -- as they are in every file that was parsed from text; here every value follows its joint.  With
`positions=True` on an `Anim` that holds End Sites the reference writes a CHANNELS line into the End Site blocks; here they get none."""
import ctypes as C
import os
from dataclasses import dataclass, field
from typing import Optional

import numpy as np
import torch

from .. import _native as N

_NO_CPU = "{} runs on the GPU only (no CPU fallback); move the motion to cuda"
_AXIS = {"Xrotation": "x", "Yrotation": "y", "Zrotation": "z"}
_AXIS_INV = {v: k for k, v in _AXIS.items()}
_POS = ("Xposition", "Yposition", "Zposition")
WRITE_ORDERS = {"zyx": 0, "xzy": 1}          # the file orders whose reverse `q2eul` (utils/rotation.py:364-382) has formulas for
END_SITE = "End Site"
FIT_FRAME_TIME = 1 / 20                      # what fit_joints_bvh hands to save_bvh


# ------------------------------------------------------------------------------------------ the hierarchy
@dataclass
class BvhSkeleton:
    """A file's hierarchy in file order, End Sites included as joints named 'End Site' and marked in `is_end`.  `rot_col` / `pos_col`: per
    joint the column of its first rotation / position channel in a frame row, -1 for none.  `order`: the rotation order read from the file
    ('zyx': Zrotation Yrotation Xrotation).  A skeleton made by `writer_skeleton` holds no End Site joints: `leaf_offsets` then are the
    offsets of the End Site blocks the writer puts under every leaf (None: zeros)."""
    names: list
    parents: list
    offsets: np.ndarray
    is_end: list
    order: str
    frametime: float
    rot_col: list
    pos_col: list
    channels: int
    leaf_offsets: Optional[np.ndarray] = None

    @property
    def joints(self):
        return len(self.names)

    @property
    def end_offsets(self):
        return self.offsets[[j for j, e in enumerate(self.is_end) if e]]

    @property
    def not_end_index(self):
        return [j for j, e in enumerate(self.is_end) if not e]

    @property
    def simple_names(self):
        return [self.names[j] for j in self.not_end_index]

    @property
    def simple_parents(self):
        """Parents among the joints that are no End Sites (bvh_utils.py:229-231)."""
        keep = self.not_end_index
        return [-1 if self.parents[j] < 0 else keep.index(self.parents[j]) for j in keep]

    def same_hierarchy(self, other):
        return (self.names == other.names and self.parents == other.parents and self.is_end == other.is_end and self.order == other.order
                and self.rot_col == other.rot_col and self.pos_col == other.pos_col and np.array_equal(self.offsets, other.offsets))


def _check_order(what, order):
    order = str(order).lower()
    if sorted(order) != ["x", "y", "z"]:
        raise ValueError(f"{what}: rotation order {order!r} is no permutation of 'xyz'")
    return order


def parse_bvh(path_or_text, start=None, end=None):
    """A BVH file (a path, or its text: anything with a line break in it) -> (BvhSkeleton, channels float32 [T, C]).
    Accepted, as by `read_bvh`: a root with 6 channels and the other joints with 3, or 6 channels on every joint.  `start` / `end` select
    frame rows with the reference's arithmetic (bvh_utils.py:165-189; 0 counts as not given).
    ValueError, naming the line: the nine-channel variant (any count but 3 and 6), a rotation order that differs between joints, position
    channels not in X, Y, Z order, a frame row with the wrong number of values, a `Frames:` count that disagrees with the rows."""
    text = path_or_text
    if isinstance(text, bytes):
        text = text.decode()
    if not isinstance(text, str) or "\n" not in text:
        with open(os.fspath(path_or_text), "r") as fh:
            text = fh.read()
    names, parents, offsets, is_end, rot_col, pos_col = [], [], [], [], [], []
    order, frametime, declared, active, col = None, None, None, -1, 0
    rows, frames_line = [], None
    lines = text.split("\n")
    for no, line in enumerate(lines, 1):
        tok = line.split()
        if not tok:
            continue
        head = tok[0]
        if declared is not None and frametime is not None:       # the motion block
            if len(tok) != col:
                raise ValueError(f"parse_bvh: line {no}: a frame row of {len(tok)} values, the hierarchy declares {col} channels")
            rows.append(tok)
        elif head in ("HIERARCHY", "MOTION", "{"):
            continue
        elif head in ("ROOT", "JOINT") or tok[:2] == ["End", "Site"]:
            if head == "ROOT" and names:
                raise ValueError(f"parse_bvh: line {no}: a second ROOT")
            if head != "ROOT" and active < 0:
                raise ValueError(f"parse_bvh: line {no}: {line.strip()!r} outside the ROOT's block")
            names.append(END_SITE if head == "End" else tok[1])
            parents.append(active)
            offsets.append([0.0, 0.0, 0.0])
            is_end.append(head == "End")
            rot_col.append(-1)
            pos_col.append(-1)
            active = len(names) - 1
        elif head == "}":
            active = parents[active]
        elif head == "OFFSET":
            if len(tok) != 4:
                raise ValueError(f"parse_bvh: line {no}: OFFSET takes three numbers")
            offsets[active] = [float(v) for v in tok[1:]]
        elif head == "CHANNELS":
            n = int(tok[1])
            if n not in (3, 6):
                raise ValueError(f"parse_bvh: line {no}: CHANNELS {n}: only 3 (rotations) and 6 (positions and rotations) are read"
                                 + (" -- the nine-channel variant is not covered" if n == 9 else ""))
            if len(tok) != 2 + n:
                raise ValueError(f"parse_bvh: line {no}: CHANNELS {n} names {len(tok) - 2} channels")
            if is_end[active] or rot_col[active] >= 0:
                raise ValueError(f"parse_bvh: line {no}: a second CHANNELS line for {names[active]!r}")
            kinds = tok[2:]
            rot = [k for k in kinds if k in _AXIS]
            pos = [k for k in kinds if k in _POS]
            if len(rot) != 3 or len(rot) + len(pos) != n:
                raise ValueError(f"parse_bvh: line {no}: channels {kinds}: three rotations and, with 6, three positions are expected")
            r0 = kinds.index(rot[0])
            if kinds[r0:r0 + 3] != rot:
                raise ValueError(f"parse_bvh: line {no}: the rotation channels are not adjacent")
            this = "".join(_AXIS[k] for k in rot)
            if sorted(this) != ["x", "y", "z"]:
                raise ValueError(f"parse_bvh: line {no}: rotation order {this!r} names an axis twice")
            if order is not None and this != order:
                raise ValueError(f"parse_bvh: line {no}: rotation order {this!r} differs from {order!r} of the joints before")
            order = this
            if pos:
                p0 = kinds.index(pos[0])
                if tuple(kinds[p0:p0 + 3]) != _POS:
                    raise ValueError(f"parse_bvh: line {no}: position channels {pos} are not in X, Y, Z order")
                pos_col[active] = col + p0
            rot_col[active] = col + r0
            col += n
        elif head == "Frames:":
            declared, frames_line = int(tok[1]), no
        elif head == "Frame" and len(tok) == 3 and tok[1] == "Time:":
            frametime = float(tok[2])
        else:
            raise ValueError(f"parse_bvh: line {no}: {line.strip()!r} is not understood")
    if not names or declared is None or frametime is None:
        raise ValueError("parse_bvh: no hierarchy, `Frames:` or `Frame Time:` line")
    for j, name in enumerate(names):
        if not is_end[j] and rot_col[j] < 0:
            raise ValueError(f"parse_bvh: joint {name!r} has no CHANNELS line")
    if declared != len(rows):
        raise ValueError(f"parse_bvh: line {frames_line}: `Frames: {declared}` but {len(rows)} frame rows follow")
    s = int(start) if start else 0
    if start and end:
        want = int(end - start)
    elif start:
        want = declared - int(start)
    elif end:
        want = int(end)
    else:
        want = declared
    rows = rows[s:int(end)] if end else rows[s:]
    if len(rows) != want or want < 1:
        raise ValueError(f"parse_bvh: start {start} and end {end} select {len(rows)} of the {declared} frames, the reference's count is {want}")
    channels = np.array(rows, dtype=np.float64).astype(np.float32).reshape(len(rows), col)
    sk = BvhSkeleton(names, parents, np.asarray(offsets, np.float64).astype(np.float32), is_end, order, frametime, rot_col, pos_col, col)
    return sk, channels


# ------------------------------------------------------------------------------------------ the writer
def writer_sequence(parents):
    """The reference's `save_joint_seq` (bvh_utils.py:571-575, :735-770): depth first from joint 0, children in index order."""
    parents = [int(p) for p in parents]
    seq = [0]

    def walk(i):
        seq.append(i)
        for j in range(len(parents)):
            if parents[j] == i:
                walk(j)

    for i in range(len(parents)):
        if parents[i] == 0:
            walk(i)
    if sorted(seq) != list(range(len(parents))):
        raise ValueError(f"writer_sequence: parents {parents} are no tree rooted at joint 0 (the writer would reach joints {sorted(seq)})")
    return seq


def writer_skeleton(names, parents, offsets, end_offsets=None, order="zyx", positions=False, frametime=1 / 24):
    """The skeleton `format_bvh` writes for joints given the way `save_bvh` gets them: in any order (the file holds them depth first,
    `writer_sequence`), with names that may hold 'End Site' entries (an `Anim` read with end_sites=True: written as End Site blocks) or
    none (an End Site block is added under every leaf, taking `end_offsets` in that order; None: zeros)."""
    order = _check_order("writer_skeleton", order)
    parents = [int(p) for p in parents]
    J = len(parents)
    names = [f"joint_{i}" for i in range(J)] if names is None else list(names)
    offsets = np.asarray(offsets, np.float32)
    if len(names) != J or offsets.shape != (J, 3):
        raise ValueError(f"writer_skeleton: {len(names)} names and offsets of shape {offsets.shape} for {J} parents")
    seq = writer_sequence(parents)
    is_end = [names[j] == END_SITE for j in seq]
    leaves = [j for j in range(J) if j not in parents]
    leaf = None
    if not any(is_end) and end_offsets is not None:
        leaf = np.asarray(end_offsets, np.float32).reshape(-1, 3)
        if len(leaf) < len(leaves):
            raise ValueError(f"writer_skeleton: {len(leaf)} end offsets for {len(leaves)} leaves")
    rot_col, pos_col, col = [], [], 0
    for k, e in enumerate(is_end):
        if e:
            rot_col.append(-1)
            pos_col.append(-1)
            continue
        six = positions or k == 0
        pos_col.append(col if six else -1)
        rot_col.append(col + 3 if six else col)
        col += 6 if six else 3
    sk = BvhSkeleton([names[j] for j in seq], [-1 if parents[j] < 0 else seq.index(parents[j]) for j in seq], offsets[seq], is_end, order,
                     float(frametime), rot_col, pos_col, col, leaf)
    return sk, seq


def format_bvh(skeleton, channels, frametime=None):
    """-> the file's text, written exactly as `save_bvh` / `save_joint` write it: depth first, tabs, `OFFSET %f %f %f`, the trailing space
    after a 6-channel CHANNELS line, an End Site block under every leaf (a skeleton without End Site joints) or the End Site joints
    themselves, `"%f "` per value and one line break per frame.  channels: [T, skeleton.channels], in the skeleton's joint order -- for a
    `writer_skeleton` that is its `writer_sequence`, which `quats_to_channels` applies."""
    sk = skeleton
    ch = np.asarray(channels, np.float32)
    if ch.ndim != 2 or ch.shape[1] != sk.channels:
        raise ValueError(f"format_bvh: channels of shape {ch.shape}, expected [T, {sk.channels}]")
    o = [_AXIS_INV[a] for a in _check_order("format_bvh", sk.order)]
    with_end = any(sk.is_end)
    leaf = sk.leaf_offsets
    taken = [0]
    out = []
    children = [[j for j in range(sk.joints) if sk.parents[j] == i] for i in range(sk.joints)]
    if sk.parents[0] != -1 or any(not 0 <= sk.parents[j] < j for j in range(1, sk.joints)):
        raise ValueError("format_bvh: the skeleton's joints are not in file order (parents[0] = -1, parents[j] < j)")

    def joint(i, t):
        if i == 0:
            out.append("%sROOT %s\n" % (t, sk.names[0]))
        elif sk.is_end[i]:
            out.append("%s%s\n" % (t, END_SITE))
        else:
            out.append("%sJOINT %s\n" % (t, sk.names[i]))
        out.append("%s{\n" % t)
        t += "\t"
        out.append("%sOFFSET %f %f %f\n" % (t, sk.offsets[i, 0], sk.offsets[i, 1], sk.offsets[i, 2]))
        if not sk.is_end[i]:
            if sk.pos_col[i] >= 0:
                out.append("%sCHANNELS 6 Xposition Yposition Zposition %s %s %s \n" % (t, o[0], o[1], o[2]))
            else:
                out.append("%sCHANNELS 3 %s %s %s\n" % (t, o[0], o[1], o[2]))
        for j in children[i]:
            joint(j, t)
        if not with_end and not children[i] and i:
            out.append("%sEnd Site\n" % t)
            out.append("%s{\n" % t)
            e = (0.0, 0.0, 0.0) if leaf is None else leaf[taken[0]]
            taken[0] += 1
            out.append("%s\tOFFSET %f %f %f\n" % (t, e[0], e[1], e[2]))
            out.append("%s}\n" % t)
        out.append("%s}\n" % t[:-1])

    expect = 0
    for i in range(sk.joints):
        if sk.is_end[i]:
            continue
        want_pos = sk.pos_col[i] >= 0
        if (want_pos and (sk.pos_col[i] != expect or sk.rot_col[i] != expect + 3)) or (not want_pos and sk.rot_col[i] != expect):
            raise ValueError("format_bvh: the skeleton's channel columns are not the ones a file written in this joint order has")
        expect += 6 if want_pos else 3
    out.append("HIERARCHY\n")
    joint(0, "")
    out.append("MOTION\n")
    out.append("Frames: %i\n" % ch.shape[0])
    out.append("Frame Time: %f\n" % (sk.frametime if frametime is None else frametime))
    row = "%f " * ch.shape[1] + "\n"
    out.extend(row % tuple(r) for r in ch.astype(np.float64).tolist())
    return "".join(out)


# ------------------------------------------------------------------------------------------ the animation object
class Anim:
    """The reference's `Anim` (bvh_utils.py:29-81): local quaternions [T, J, 4], local positions [T, J, 3], offsets [J, 3], parents, bone
    names, the End Sites' offsets."""

    def __init__(self, quats, pos, offsets, parents, bones=None, end_offsets=None):
        self.quats, self.pos, self.offsets, self.parents = quats, pos, offsets, parents
        self.bones = [f"joint_{i}" for i in range(len(parents))] if bones is None else bones
        self.end_offsets = end_offsets
        self.not_endsite = [i for i, b in enumerate(self.bones) if b != END_SITE]
        self.endsite = [i for i, b in enumerate(self.bones) if b == END_SITE]

    @property
    def shape(self):
        return (self.quats.shape[0], self.quats.shape[1])

    def clip(self, slice):
        self.quats = self.quats[slice]
        self.pos = self.pos[slice]


@dataclass
class BvhMotion:
    """What `decode_channels` / `load_bvh` return.  rotations [B, T', J, 4] (w, x, y, z) and positions [B, T', J, 3] (global) are what
    `encode_joints(positions, rotations, mode="posrot")` takes; lengths int32 [B]: the frames of each clip after sub-sampling, every later
    row exact zeros.  joints: the file joint of every output joint; parents: among the output joints (-1: no selected ancestor).
    local_positions (`Anim.pos`) and global_rotations are None unless asked for."""
    positions: torch.Tensor
    rotations: torch.Tensor
    lengths: torch.Tensor
    skeleton: BvhSkeleton
    joints: list = field(default_factory=list)
    parents: list = field(default_factory=list)
    local_positions: Optional[torch.Tensor] = None
    global_rotations: Optional[torch.Tensor] = None


# ------------------------------------------------------------------------------------------ the launches
def max_joints():
    """Most file joints, End Sites included (mst_bvh_max_joints)."""
    return int(N.lib().mst_bvh_max_joints())


def max_frames(joints):
    """Longest clip `decode_channels` takes (mst_bvh_max_frames)."""
    n = int(N.lib().mst_bvh_max_frames(int(joints)))
    if n < 0:
        N.check(1)
    return n


def _ints(v):
    return (C.c_int32 * max(len(v), 1))(*[int(a) for a in v])


def _select(what, skeleton, joints):
    """-> (file joints, parents among them)."""
    if joints is None:
        return list(range(skeleton.joints)), list(skeleton.parents)
    sel = []
    for j in joints:
        if isinstance(j, str):
            if skeleton.names.count(j) != 1:
                raise ValueError(f"{what}: joint {j!r} is named {skeleton.names.count(j)} times in the file")
            j = skeleton.names.index(j)
        j = int(j)
        if not 0 <= j < skeleton.joints:
            raise ValueError(f"{what}: selected joint {j} outside 0..{skeleton.joints - 1}")
        if j in sel:
            raise ValueError(f"{what}: joint {j} is selected twice")
        sel.append(j)
    if not 1 <= len(sel) <= 24:
        raise ValueError(f"{what}: {len(sel)} selected joints outside 1..24")
    par = []
    for j in sel:
        a = skeleton.parents[j]
        while a >= 0 and a not in sel:
            a = skeleton.parents[a]
        par.append(sel.index(a) if a >= 0 else -1)
    return sel, par


def _rate(what, downsample_rate, phase):
    if downsample_rate is None:
        stride = 1
    else:
        if round(downsample_rate) != downsample_rate:
            raise NotImplementedError(f"{what}: a fractional downsample_rate ({downsample_rate}) is the reference's slerp up-sampling path, "
                                      "which is not covered")
        stride = int(downsample_rate)
    if stride < 1:
        raise ValueError(f"{what}: downsample_rate {downsample_rate} < 1")
    if not 0 <= int(phase) < stride:
        raise ValueError(f"{what}: phase {phase} outside 0..{stride - 1}")
    return stride, int(phase)


def decode_channels(channels, skeleton, lengths=None, joints=None, scale=1.0, downsample_rate=None, phase=0, return_local=False,
                    return_global=False):
    """Channel values [B, T, C] (CUDA float32; what `parse_bvh` returns, padded to one T) of clips that share `skeleton` -> BvhMotion, one
    launch on the caller's current stream.  lengths [B]: a clip's own frames, 1 <= len <= T (checked on the host).  joints: up to 24 file
    joints (indices or names) in the model's order -- a selected joint's rotation is relative to its nearest selected ancestor, so
    skipped joints fold in; None: every file joint, End Sites included, and the rotations are the reference's `Anim.quats`.
    scale: applied to offsets and position channels.  downsample_rate k, phase i: frames i, i + k, ... of each clip, the signs made
    continuous over the full-rate frames first, as in the reference.  The input is not modified."""
    what = "decode_channels"
    if not torch.is_tensor(channels):
        raise TypeError(f"{what}: channels is a tensor (load_bvh takes paths, read_bvh a file)")
    if channels.dim() != 3 or channels.shape[-1] != skeleton.channels:
        raise ValueError(f"{what}: channels of shape {tuple(channels.shape)}, expected [B, T, {skeleton.channels}]")
    B, T, Cn = channels.shape
    Jf = skeleton.joints
    stride, phase = _rate(what, downsample_rate, phase)
    order = _check_order(what, skeleton.order)
    sel, par = _select(what, skeleton, joints)
    if B < 1 or T < 1:
        raise ValueError(f"{what}: {B} clips of {T} frames")
    if phase >= T:
        raise ValueError(f"{what}: phase {phase} leaves no frame of {T}")
    host = None
    if lengths is not None:
        host = lengths.detach().cpu().numpy() if torch.is_tensor(lengths) else np.asarray(lengths)
        host = host.reshape(-1).astype(np.int64)
        if host.shape[0] != B:
            raise ValueError(f"{what}: {host.shape[0]} lengths for {B} clips")
        if host.min() < 1 or host.max() > T:
            raise ValueError(f"{what}: lengths {host.min()}..{host.max()} outside 1..{T}")
    if not channels.is_cuda or (torch.is_tensor(lengths) and not lengths.is_cuda):
        raise RuntimeError(_NO_CPU.format(what))
    if Jf > max_joints():
        raise ValueError(f"{what}: {Jf} file joints (End Sites included) > {max_joints()} (mst_bvh_max_joints)")
    if T > max_frames(Jf):
        raise RuntimeError(f"{what}: {T} frames > {max_frames(Jf)}, the longest clip mst_bvh_decode takes (mst_bvh_max_frames({Jf})); read the "
                           "file in pieces (start / end)")
    dev = channels.device
    ch = channels.detach().to(torch.float32).contiguous()
    ld = None if host is None else torch.from_numpy(host.astype(np.int32)).to(dev)
    J = len(sel)
    Tout = (T - phase + stride - 1) // stride
    new = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
    ws, rot, pos = new(B, T, Jf, 11), new(B, Tout, J, 4), new(B, Tout, J, 3)
    lpos = new(B, Tout, J, 3) if return_local else None
    grot = new(B, Tout, J, 4) if return_global else None
    offs = (C.c_float * (3 * Jf))(*np.asarray(skeleton.offsets, np.float32).reshape(-1).tolist())
    with torch.cuda.device(dev):
        N.check(N.lib().mst_bvh_decode(N.ptr(ch), N.ptr(ld), B, T, Cn, Jf, _ints(skeleton.parents), _ints(skeleton.rot_col),
                                       _ints(skeleton.pos_col), offs, _ints(["xyz".index(a) for a in order]), float(scale), stride, phase,
                                       None if joints is None else _ints(sel), 0 if joints is None else J, N.ptr(ws), N.ptr(rot), N.ptr(pos),
                                       N.ptr(lpos), N.ptr(grot), N.stream_ptr(dev)))
    full = np.full(B, T, np.int64) if host is None else host
    out_len = np.maximum((full - phase + stride - 1) // stride, 0).astype(np.int32)
    return BvhMotion(pos, rot, torch.from_numpy(out_len).to(dev), skeleton, sel, par, lpos, grot)


def load_bvh(paths, joints=None, scale=1.0, downsample_rate=None, phase=0, start=None, end=None, device="cuda"):
    """BVH files of one hierarchy -> BvhMotion: every file parsed on the host, the clips padded to the longest, uploaded once and decoded in
    one launch (`decode_channels` has the arguments)."""
    if isinstance(paths, (str, bytes, os.PathLike)):
        paths = [paths]
    paths = list(paths)
    if not paths:
        raise ValueError("load_bvh: no files")
    parsed = [parse_bvh(p, start, end) for p in paths]
    sk = parsed[0][0]
    for p, (other, _) in zip(paths[1:], parsed[1:]):
        if not sk.same_hierarchy(other):
            raise ValueError(f"load_bvh: {p} does not share the hierarchy (names, parents, offsets, channels) of {paths[0]}")
    lengths = np.array([len(c) for _, c in parsed], np.int32)
    batch = np.zeros((len(parsed), int(lengths.max()), sk.channels), np.float32)
    for b, (_, c) in enumerate(parsed):
        batch[b, :len(c)] = c
    stride, phase = _rate("load_bvh", downsample_rate, phase)
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError(_NO_CPU.format("load_bvh"))
    return decode_channels(torch.from_numpy(batch).to(dev), sk, lengths, joints, scale, stride, phase)


def read_bvh(filename, start=None, end=None, order=None, downsample_rate=None, end_sites=False):
    """The reference's `read_bvh`, signature and return: an `Anim` of numpy arrays -- quats [T, J, 4], pos [T, J, 3], offsets, parents,
    bones, end_offsets -- without the End Sites unless `end_sites`; for an integer `downsample_rate` k a list of k of them, one per phase
    (without end_offsets, as there).  order: overrides the rotation order read from the file.  The conversion runs on the GPU."""
    if downsample_rate is not None:
        _rate("read_bvh", downsample_rate, 0)
    sk, ch = parse_bvh(filename, start, end)
    if order is not None:
        sk.order = _check_order("read_bvh", order)
    if not torch.cuda.is_available():
        raise RuntimeError(_NO_CPU.format("read_bvh"))
    m = decode_channels(torch.from_numpy(ch).cuda()[None], sk, return_local=True)
    quats, pos = m.rotations[0].cpu().numpy(), m.local_positions[0].cpu().numpy()
    keep = list(range(sk.joints)) if end_sites else sk.not_end_index
    offsets = sk.offsets if end_sites else sk.offsets[keep]
    parents = np.array(sk.parents if end_sites else sk.simple_parents)
    bones = list(sk.names) if end_sites else sk.simple_names

    def anim(sl, end_offsets):
        return Anim(quats[sl][:, keep], pos[sl][:, keep], offsets, parents, bones, end_offsets)

    if downsample_rate is None:
        return anim(slice(None), sk.end_offsets)
    k = int(downsample_rate)
    return [anim(slice(i, None, k), None) for i in range(k)]


def read_bvh_resampled(filename, downsample_rate, start=None, end=None, end_sites=False):
    """The reference's `read_bvh` for a fractional `downsample_rate` (bvh_utils.py:251-287), e.g. 1.5 for a 30 fps file read at 20 fps: a
    list of one `Anim` of numpy arrays, as there -- the local quaternions through `qslerp` and the local positions through `lerp`, both
    float32, ceil((T - 1) * up / down) frames (the file's last frame is dropped, as there), without end_offsets.  The rate is read as the
    reference's `decimal_to_fraction` reads it, from the number's own decimal text (1.5 -> 3/2); a `Fraction` or an (int, int) pair is taken
    as it is.  The quaternions are made sign-continuous first (`decode_channels`), so the reference's formula (`shortest=False`) already
    follows the shorter arc.  Global positions after the resampling are not formed: that is a forward-kinematics pass over the result."""
    from fractions import Fraction
    from . import pose_track as pt
    what = "read_bvh_resampled"
    if isinstance(downsample_rate, (Fraction, tuple, list)):
        rate = pt.parse_rate(downsample_rate)
    else:
        rate = pt.parse_rate(pt.decimal_to_fraction(downsample_rate))
    sk, ch = parse_bvh(filename, start, end)
    if len(ch) < 2:
        raise ValueError(f"{what}: {len(ch)} frame; a file is resampled interval by interval, so 2 frames at least")
    if not torch.cuda.is_available():
        raise RuntimeError(_NO_CPU.format(what))
    m = decode_channels(torch.from_numpy(ch).cuda()[None], sk, return_local=True)
    quats, pos, _ = pt.resample_tracks(m.rotations, m.local_positions, rate=rate, shortest=False)
    quats, pos = quats[0].cpu().numpy(), pos[0].cpu().numpy()
    if end_sites:
        return [Anim(quats, pos, sk.offsets, np.array(sk.parents), list(sk.names))]
    keep = sk.not_end_index
    return [Anim(quats[:, keep], pos[:, keep], sk.offsets[keep], np.array(sk.simple_parents), sk.simple_names)]


def quats_to_channels(quats, root_pos, parents, order="zyx", positions=None):
    """Local quaternions [B, T, J, 4] (need not be normalised) and root positions [B, T, 3] -> the channel values `format_bvh` writes,
    [B, T, 3 + 3 J]: the root position, then per joint in the writer's order (`writer_sequence(parents)`) its Euler angles in degrees in
    the file's channel order.  positions [B, T, J, 3]: a file with `positions=True`, [B, T, 6 J].  order: 'zyx' (the reference's default and
    what every caller of it uses) or 'xzy'; the reference's `q2eul` converts no other.  `JointFit.joint_quats` and `JointFit.r_pos` are
    taken as they are.  One launch on the caller's current stream."""
    what = "quats_to_channels"
    order = _check_order(what, order)
    if order not in WRITE_ORDERS:
        raise NotImplementedError(f"{what}: order {order!r}: the reference's q2eul converts only the reverses of {tuple(WRITE_ORDERS)}")
    if not torch.is_tensor(quats) or not torch.is_tensor(root_pos) or (positions is not None and not torch.is_tensor(positions)):
        raise TypeError(f"{what}: quats, root_pos and positions are tensors (save_bvh takes the reference's numpy Anim)")
    if quats.dim() != 4 or quats.shape[-1] != 4:
        raise ValueError(f"{what}: quats of shape {tuple(quats.shape)}, expected [B, T, J, 4]")
    B, T, J, _ = quats.shape
    if tuple(root_pos.shape) != (B, T, 3):
        raise ValueError(f"{what}: root_pos of shape {tuple(root_pos.shape)}, expected [{B}, {T}, 3]")
    if positions is not None and tuple(positions.shape) != (B, T, J, 3):
        raise ValueError(f"{what}: positions of shape {tuple(positions.shape)}, expected [{B}, {T}, {J}, 3]")
    if len(parents) != J:
        raise ValueError(f"{what}: {len(parents)} parents for {J} joints")
    seq = writer_sequence(parents)
    if B < 1 or T < 1:
        raise ValueError(f"{what}: {B} clips of {T} frames")
    if any(not t.is_cuda for t in (quats, root_pos, positions) if t is not None):
        raise RuntimeError(_NO_CPU.format(what))
    if J > max_joints():
        raise ValueError(f"{what}: {J} joints > {max_joints()} (mst_bvh_max_joints)")
    dev = quats.device
    q = quats.detach().to(torch.float32).contiguous()
    r = root_pos.detach().to(device=dev, dtype=torch.float32).contiguous()
    p = None if positions is None else positions.detach().to(device=dev, dtype=torch.float32).contiguous()
    out = torch.empty(B, T, 6 * J if p is not None else 3 + 3 * J, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        N.check(N.lib().mst_quats_to_channels(N.ptr(q), N.ptr(r), N.ptr(p), _ints(seq), B, T, J, WRITE_ORDERS[order], N.ptr(out),
                                              N.stream_ptr(dev)))
    return out


def _anim_skeleton(what, anim, frametime, order, positions, end_offset):
    names = anim.bones
    J = anim.quats.shape[1]
    if J < np.shape(anim.offsets)[0]:
        raise NotImplementedError(f"{what}: an Anim whose offsets ({np.shape(anim.offsets)[0]}) include End Sites while its quaternions "
                                  f"({J}) do not is not covered")
    if names is not None and END_SITE in names:
        end_offset = None
    elif end_offset is None:
        end_offset = anim.end_offsets
    return writer_skeleton(names, anim.parents, anim.offsets, end_offset, order, positions, frametime)


def save_bvh(filename, anim, frametime=1.0 / 24.0, order="zyx", positions=False, orients=True, end_offset=None):
    """The reference's `save_bvh`, signature and defaults: `anim` is anything with quats [T, J, 4], pos [T, J, 3], offsets, parents, bones
    and end_offsets (numpy; this module's `Anim` or the reference's).  `orients` is ignored, as there.  The Euler angles come from one
    launch; `anim` is not modified (the reference permutes its quaternions in place)."""
    sk, _ = _anim_skeleton("save_bvh", anim, frametime, order, positions, end_offset)
    if not torch.cuda.is_available():
        raise RuntimeError(_NO_CPU.format("save_bvh"))
    quats = torch.as_tensor(np.asarray(anim.quats, np.float32)).cuda()[None]
    pos = torch.as_tensor(np.asarray(anim.pos, np.float32)).cuda()[None]
    ch = quats_to_channels(quats, pos[:, :, 0], anim.parents, order, pos if positions else None)[0].cpu().numpy()
    ch = _drop_end_columns(ch, sk, positions)
    with open(filename, "w") as fh:
        fh.write(format_bvh(sk, ch))


def _drop_end_columns(ch, sk, positions):
    """quats_to_channels writes a slot for every joint it is given; an Anim's End Site joints have no channels in the file."""
    if not any(sk.is_end):
        return ch
    if positions:
        keep = [c for k, e in enumerate(sk.is_end) if not e for c in range(6 * k, 6 * k + 6)]
    else:
        keep = [0, 1, 2] + [c for k, e in enumerate(sk.is_end) if not e for c in range(3 + 3 * k, 6 + 3 * k)]
    return ch[:, keep]


def save_fit(path, joint_quats, positions, real_offset, parents, names, frametime):
    """The `save=` callable `fit_joints_bvh` documents: with `fit_joints_bvh(..., save=bvh.save_fit)` the fitted animation is written by this
    package, no reference checkout needed.  What the reference's default does: `save_bvh(path, Anim(joint_quats, positions, real_offset,
    parents, names), frametime)`."""
    save_bvh(path, Anim(np.asarray(joint_quats), np.asarray(positions), np.asarray(real_offset), list(parents), names), frametime)


def save_fits(paths, fit, real_offset, parents, names=None, lengths=None, frametime=FIT_FRAME_TIME):
    """A whole `JointFit` batch written, one file per clip: one launch, one device-to-host copy, then text.  real_offset [J, 3] (row 0 is
    written as zeros, as `fit_joints_bvh` does); parents: a parents list; lengths [B]: the frames of each clip to write (None: all)."""
    from .joint_fit import _resolve_parents
    B, T, J, _ = fit.joint_quats.shape
    paths = list(paths)
    if len(paths) != B:
        raise ValueError(f"save_fits: {len(paths)} paths for {B} clips")
    parents = _resolve_parents(parents, J)
    off = np.array(real_offset, np.float32)
    if off.shape != (J, 3):
        raise ValueError(f"save_fits: offsets of shape {off.shape}, expected ({J}, 3)")
    off[0] = 0
    host = np.full(B, T, np.int64) if lengths is None else \
        (lengths.detach().cpu().numpy() if torch.is_tensor(lengths) else np.asarray(lengths)).reshape(-1).astype(np.int64)
    if host.shape[0] != B or host.min() < 1 or host.max() > T:
        raise ValueError(f"save_fits: lengths {host.tolist()} for {B} clips of {T} frames")
    sk, _ = writer_skeleton(names, parents, off, None, "zyx", False, frametime)
    ch = quats_to_channels(fit.joint_quats, fit.r_pos, parents).cpu().numpy()
    for b, p in enumerate(paths):
        with open(p, "w") as fh:
            fh.write(format_bvh(sk, ch[b, :host[b]]))
