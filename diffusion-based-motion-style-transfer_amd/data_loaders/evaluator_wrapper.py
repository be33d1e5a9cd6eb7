"""The T2M evaluators on the GPU: data_loaders/humanml/networks/evaluator_wrapper.py (`EvaluatorMDMWrapper`) over
networks/modules.py's `MovementConvEncoder`, `MotionEncoderBiGRUCo` and `TextEncoderBiGRUCo`, as a chain of native launches
(csrc/mst_eval.h): the two convolutions as GEMMs that gather their frames where they lie, the Linears, the GRU's input projections of
every step and both directions as one GEMM, one launch a time step for the recurrence, LayerNorm + LeakyReLU.  Everything is fp32 --
the evaluator is what generated clips are measured with -- and nothing falls back to torch: CPU tensors are refused.

A clip's embedding is a fixed-order sum of its own frames: it does not depend on what else is in the batch or where the clip stands in
it.  Dropout is the identity (the reference evaluates in eval mode).

    ev = MotionEvaluator.from_checkpoint('t2m/text_mot_match/model/finest.tar', dim_pose=263, device='cuda')
    emb = ev.embed_samples(sample, lengths, scale, shift)        # [B, F, 1, T] straight from a sampler, input order
    ev.get_motion_embeddings(motions, m_lens)                    # the reference's call: rows ordered by descending length
"""
import os

import numpy as np
import torch

from .. import _native as N

_NO_CPU = "{}: the evaluators run in the HIP library only (no CPU fallback): tensors must be on a GPU"
MOVEMENT_KEYS = ("main.0.weight", "main.0.bias", "main.3.weight", "main.3.bias", "out_net.weight", "out_net.bias")
GRU_KEYS = tuple(f"gru.{n}_l0{r}" for r in ("", "_reverse") for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"))
OUTPUT_KEYS = ("output_net.0.weight", "output_net.0.bias", "output_net.1.weight", "output_net.1.bias", "output_net.3.weight",
               "output_net.3.bias", "hidden")
MOTION_KEYS = ("input_emb.weight", "input_emb.bias") + GRU_KEYS + OUTPUT_KEYS
TEXT_KEYS = ("pos_emb.weight", "pos_emb.bias") + MOTION_KEYS
LN_EPS = 1e-5


def conv_frames(T):
    """Frames a Conv1d(., ., 4, 2, 1) yields for T."""
    return (T - 2) // 2 + 1 if T >= 2 else 0


def movement_frames(T):
    """Movement frames of a clip of T frames: two such convolutions."""
    return conv_frames(conv_frames(T))


def align_index(m_lens):
    """The reference's row order: descending length, ties as numpy's argsort leaves them reversed."""
    return np.argsort(_host_ints(m_lens).tolist())[::-1].copy()


def _host_ints(v):
    if torch.is_tensor(v):
        v = v.detach().cpu().numpy()
    return np.asarray(v).astype(np.int64).reshape(-1)


def _f32(t):
    t = t if torch.is_tensor(t) else torch.as_tensor(np.asarray(t))
    return t.detach().to(torch.float32)


def pack_movement(sd):
    """State dict of a MovementConvEncoder -> fp32 tensors in the layout the GEMM reads: the conv weights [out, in, 4] as
    [out, 4 * in] with k = tap * in + channel."""
    missing = [k for k in MOVEMENT_KEYS if k not in sd]
    if missing:
        raise KeyError(f"movement_encoder: missing {missing}")
    out = {}
    for name, key in (("conv1", "main.0"), ("conv2", "main.3")):
        w = _f32(sd[key + ".weight"])
        if w.dim() != 3 or w.shape[2] != 4:
            raise ValueError(f"movement_encoder: {key}.weight of shape {tuple(w.shape)}, expected [out, in, 4]")
        out[name + "_w"] = w.permute(0, 2, 1).reshape(w.shape[0], 4 * w.shape[1]).contiguous()
        out[name + "_b"] = _f32(sd[key + ".bias"]).contiguous()
    out["out_w"] = _f32(sd["out_net.weight"]).contiguous()
    out["out_b"] = _f32(sd["out_net.bias"]).contiguous()
    if out["conv2_w"].shape[1] != 4 * out["conv1_w"].shape[0] or out["out_w"].shape[1] != out["conv2_w"].shape[0]:
        raise ValueError("movement_encoder: the layers' widths do not chain")
    return out


def pack_recurrent(sd, what, text=False):
    """State dict of a MotionEncoderBiGRUCo / TextEncoderBiGRUCo -> fp32 tensors: w_ih [6 H, H] and b_ih [6 H] (forward rows, then
    `_reverse`), w_hh [2, 3 H, H], b_hh [2, 3 H], hidden [2, H], and the Linears as they are."""
    keys = TEXT_KEYS if text else MOTION_KEYS
    missing = [k for k in keys if k not in sd]
    if missing:
        raise KeyError(f"{what}: missing {missing}")
    g = lambda n: _f32(sd[n])
    H = g("gru.weight_hh_l0").shape[1]
    for r in ("", "_reverse"):
        if tuple(g(f"gru.weight_hh_l0{r}").shape) != (3 * H, H) or tuple(g(f"gru.weight_ih_l0{r}").shape) != (3 * H, H):
            raise ValueError(f"{what}: gru weights{r} are not [3 H, H] at H = {H}")
    if H % 64:
        raise ValueError(f"{what}: hidden width {H} is no multiple of 64")
    out = dict(
        in_w=g("input_emb.weight").contiguous(), in_b=g("input_emb.bias").contiguous(),
        w_ih=torch.cat([g("gru.weight_ih_l0"), g("gru.weight_ih_l0_reverse")], 0).contiguous(),
        b_ih=torch.cat([g("gru.bias_ih_l0"), g("gru.bias_ih_l0_reverse")], 0).contiguous(),
        w_hh=torch.stack([g("gru.weight_hh_l0"), g("gru.weight_hh_l0_reverse")], 0).contiguous(),
        b_hh=torch.stack([g("gru.bias_hh_l0"), g("gru.bias_hh_l0_reverse")], 0).contiguous(),
        hidden=g("hidden").reshape(2, H).contiguous(),
        o0_w=g("output_net.0.weight").contiguous(), o0_b=g("output_net.0.bias").contiguous(),
        ln_w=g("output_net.1.weight").contiguous(), ln_b=g("output_net.1.bias").contiguous(),
        o3_w=g("output_net.3.weight").contiguous(), o3_b=g("output_net.3.bias").contiguous())
    if tuple(out["in_w"].shape)[0] != H or tuple(out["o0_w"].shape) != (H, 2 * H) or out["o3_w"].shape[1] != H or g("hidden").numel() != 2 * H:
        raise ValueError(f"{what}: the layers' widths do not chain at H = {H}")
    if text:
        out["pos_w"] = g("pos_emb.weight").contiguous()
        out["pos_b"] = g("pos_emb.bias").contiguous()
        if out["pos_w"].shape[0] != out["in_w"].shape[1]:
            raise ValueError(f"{what}: pos_emb yields {out['pos_w'].shape[0]} features, input_emb reads {out['in_w'].shape[1]}")
    return out


class MotionEvaluator:
    """The three evaluator networks, uploaded once as fp32.  State dicts carry the reference's key names (`main.0.weight`,
    `gru.weight_hh_l0_reverse`, `output_net.3.bias`, `hidden`, ...)."""

    def __init__(self, movement_encoder, motion_encoder, text_encoder=None, *, dim_pose, unit_length=4, device):
        self.device = torch.device(device)
        self.dim_pose = int(dim_pose)
        self.unit_length = int(unit_length)
        to = lambda d: {k: v.to(self.device) for k, v in d.items()}
        self.movement = to(pack_movement(movement_encoder))
        self.motion = to(pack_recurrent(motion_encoder, "motion_encoder"))
        self.text = None if text_encoder is None else to(pack_recurrent(text_encoder, "text_encoder", text=True))
        C = self.movement["conv1_w"].shape[1] // 4
        if C != self.dim_pose - 4:
            raise ValueError(f"MotionEvaluator: the movement encoder reads {C} features, dim_pose - 4 = {self.dim_pose - 4}")
        if self.motion["in_w"].shape[1] != self.movement["out_w"].shape[0]:
            raise ValueError("MotionEvaluator: the motion encoder does not read the movement encoder's width")

    @classmethod
    def from_checkpoint(cls, path, *, dim_pose, unit_length=4, device, text=True):
        """The `finest.tar` layout: keys `movement_encoder`, `text_encoder`, `motion_encoder`."""
        ck = torch.load(path, map_location="cpu")
        return cls(ck["movement_encoder"], ck["motion_encoder"], ck["text_encoder"] if text else None, dim_pose=dim_pose,
                   unit_length=unit_length, device=device)

    # ---------------------------------------------------------------------------------------- checks (no GPU needed)
    def _steps(self, what, m_lens, B, T):
        lens = _host_ints(m_lens)
        if lens.shape[0] != B:
            raise ValueError(f"{what}: {lens.shape[0]} lengths for {B} clips")
        if T < 4:
            raise ValueError(f"{what}: {T} frames: the two convolutions need at least 4")
        steps = lens // self.unit_length
        if (lens < 0).any() or (steps == 0).any():
            raise ValueError(f"{what}: a length below unit_length = {self.unit_length} leaves no movement frame "
                             "(pack_padded_sequence raises there)")
        most = movement_frames(T)
        if (steps > most).any():
            raise ValueError(f"{what}: length {int(lens.max())} asks for {int(steps.max())} movement frames, {T} frames yield {most}")
        return steps

    def _check_feats(self, what, feats):
        if feats != self.dim_pose:
            raise ValueError(f"{what}: {feats} features, the evaluator reads {self.dim_pose}")

    # ---------------------------------------------------------------------------------------- launches
    def _gemm(self, a, w, bias, M, *, lda=0, add=None, leaky=False, mode=0, batch=0, frames=0, channels=0, ldx=0, sb=0, scale=None,
              shift=None):
        Nn, K = w.shape
        c = torch.empty(M, Nn, dtype=torch.float32, device=a.device)
        N.check(N.lib().mst_eval_gemm(N.ptr(a), N.ptr(w), N.ptr(bias), N.ptr(add), N.ptr(c), M, Nn, K, lda or K, Nn,
                                      0 if add is None else add.shape[-1], mode, batch, frames, channels, ldx, sb, N.ptr(scale), N.ptr(shift),
                                      int(leaky), N.stream_ptr(a.device)))
        return c

    def _recurrent(self, net, x, B, Tm, steps):
        """x [B * Tm, H_in] -> [B, out]: input projections of every position, the recurrence, the output net."""
        H = net["w_hh"].shape[2]
        dev = x.device
        xproj = self._gemm(x, net["w_ih"], net["b_ih"], B * Tm)
        steps_dev = torch.as_tensor(np.ascontiguousarray(steps, dtype=np.int32)).to(dev)
        work = torch.empty(2, B, 2 * H, dtype=torch.float32, device=dev)
        last = torch.empty(B, 2 * H, dtype=torch.float32, device=dev)
        N.check(N.lib().mst_eval_gru(N.ptr(xproj), N.ptr(net["w_hh"]), N.ptr(net["b_hh"]), N.ptr(net["hidden"]), N.ptr(steps_dev), B, Tm, H,
                                     int(steps.max()), N.ptr(work), N.ptr(last), N.stream_ptr(dev)))
        y = self._gemm(last, net["o0_w"], net["o0_b"], B)
        z = torch.empty_like(y)
        N.check(N.lib().mst_eval_layernorm(N.ptr(y), N.ptr(net["ln_w"]), N.ptr(net["ln_b"]), N.ptr(z), B, H, LN_EPS, 1, N.stream_ptr(dev)))
        return self._gemm(z, net["o3_w"], net["o3_b"], B)

    def _embed(self, what, x, sampler, steps, scale, shift):
        if not x.is_cuda or not self.movement["conv1_w"].is_cuda:
            raise RuntimeError(_NO_CPU.format(what))
        mv, F = self.movement, self.dim_pose
        B, T = (x.shape[0], x.shape[3]) if sampler else (x.shape[0], x.shape[1])
        T1, T2 = conv_frames(T), movement_frames(T)
        C = F - 4
        with torch.cuda.device(x.device):
            y1 = self._gemm(x, mv["conv1_w"], mv["conv1_b"], B * T1, leaky=True, mode=2 if sampler else 1, batch=B, frames=T, channels=C,
                            ldx=F, sb=F * T, scale=scale, shift=shift)
            H1 = y1.shape[1]
            y2 = self._gemm(y1, mv["conv2_w"], mv["conv2_b"], B * T2, leaky=True, mode=1, batch=B, frames=T1, channels=H1, ldx=H1, sb=T1 * H1)
            mov = self._gemm(y2, mv["out_w"], mv["out_b"], B * T2)
            emb = self._gemm(mov, self.motion["in_w"], self.motion["in_b"], B * T2)
            return self._recurrent(self.motion, emb, B, T2, steps)

    def _affine(self, what, scale, shift):
        if (scale is None) != (shift is None):
            raise ValueError(f"{what}: scale and shift come together")
        if scale is None:
            return None, None
        out = []
        for name, v in (("scale", scale), ("shift", shift)):
            v = _f32(v).reshape(-1)
            if v.shape[0] != self.dim_pose:
                raise ValueError(f"{what}: {name} of {v.shape[0]} entries, expected {self.dim_pose}")
            out.append(v.to(self.device).contiguous())
        return out

    # ---------------------------------------------------------------------------------------- public
    def embed_motions(self, motions, m_lens):
        """motions [B, T, dim_pose] (normalised as the evaluators were trained), m_lens [B] -> [B, out] in input order."""
        what = "embed_motions"
        if motions.dim() != 3:
            raise ValueError(f"{what}: motions of shape {tuple(motions.shape)}, expected [B, T, {self.dim_pose}]")
        self._check_feats(what, motions.shape[2])
        steps = self._steps(what, m_lens, motions.shape[0], motions.shape[1])
        x = motions.detach().to(self.device).float().contiguous()
        return self._embed(what, x, False, steps, None, None)

    def embed_samples(self, sample, lengths, scale=None, shift=None):
        """sample [B, dim_pose, 1, T] as the samplers return it, lengths [B] (host values) -> [B, out] in input order.  scale / shift
        [dim_pose]: every feature is read as x * scale + shift -- the `inv_transform` then `(x - mean_for_eval) / std_for_eval` of
        CompMDMGeneratedDataset.__getitem__ is scale = std / std_for_eval, shift = (mean - mean_for_eval) / std_for_eval.  No transpose,
        no renormalised copy: the sample is read where it lies."""
        what = "embed_samples"
        if sample.dim() != 4 or sample.shape[2] != 1:
            raise ValueError(f"{what}: sample of shape {tuple(sample.shape)}, expected [B, {self.dim_pose}, 1, T]")
        self._check_feats(what, sample.shape[1])
        steps = self._steps(what, lengths, sample.shape[0], sample.shape[3])
        scale, shift = self._affine(what, scale, shift)
        x = sample.detach().to(self.device).float().contiguous()
        return self._embed(what, x, True, steps, scale, shift)

    def embed_text(self, word_embs, pos_ohot, cap_lens):
        """word_embs [B, L, W], pos_ohot [B, L, P], cap_lens [B] in any order -> [B, out] in input order."""
        what = "embed_text"
        if self.text is None:
            raise ValueError(f"{what}: this evaluator was built without text weights")
        tx = self.text
        W, P = tx["in_w"].shape[1], tx["pos_w"].shape[1]
        if word_embs.dim() != 3 or word_embs.shape[2] != W or pos_ohot.dim() != 3 or pos_ohot.shape[2] != P or \
                tuple(pos_ohot.shape[:2]) != tuple(word_embs.shape[:2]):
            raise ValueError(f"{what}: word_embs {tuple(word_embs.shape)} / pos_ohot {tuple(pos_ohot.shape)}, expected [B, L, {W}] / [B, L, {P}]")
        B, L = word_embs.shape[:2]
        lens = _host_ints(cap_lens)
        if lens.shape[0] != B or (lens < 1).any() or (lens > L).any():
            raise ValueError(f"{what}: caption lengths {lens.tolist()} for {B} captions of {L} tokens: one each, 1..{L}")
        we = word_embs.detach().to(self.device).float().contiguous()
        po = pos_ohot.detach().to(self.device).float().contiguous()
        if not we.is_cuda:
            raise RuntimeError(_NO_CPU.format(what))
        with torch.cuda.device(we.device):
            inputs = self._gemm(po, tx["pos_w"], tx["pos_b"], B * L, add=we)
            emb = self._gemm(inputs, tx["in_w"], tx["in_b"], B * L)
            return self._recurrent(tx, emb, B, L, lens)

    def get_motion_embeddings(self, motions, m_lens):
        """The reference's call: rows in its order, `align_index(m_lens)`."""
        idx = align_index(m_lens)
        return self.embed_motions(motions, m_lens)[torch.as_tensor(idx, device=self.device)]

    def get_co_embeddings(self, word_embs, pos_ohot, cap_lens, motions, m_lens):
        """-> (text_embedding, motion_embedding), both in the reference's order.  The reference packs the captions as they come and so
        needs them sorted by descending length; here any order is taken."""
        if self.text is None:
            raise ValueError("get_co_embeddings: this evaluator was built without text weights")
        idx = torch.as_tensor(align_index(m_lens), device=self.device)
        motion = self.embed_motions(motions, m_lens)[idx]
        return self.embed_text(word_embs, pos_ohot, cap_lens)[idx], motion


class EvaluatorMDMWrapper(MotionEvaluator):
    """Drop-in for the reference's class of this name: reads <checkpoints_dir>/<t2m | dataset>/text_mot_match/model/finest.tar."""

    def __init__(self, dataset_name, device, checkpoints_dir="."):
        folder = "t2m" if dataset_name == "humanml" else dataset_name
        ck = torch.load(os.path.join(checkpoints_dir, folder, "text_mot_match", "model", "finest.tar"), map_location="cpu")
        super().__init__(ck["movement_encoder"], ck["motion_encoder"], ck["text_encoder"], dim_pose=263 if dataset_name == "humanml" else 251,
                         unit_length=4, device=device)
        self.opt = dict(dataset_name=dataset_name, device=device, dim_word=300, max_motion_length=196, dim_pos_ohot=15,
                        dim_motion_hidden=1024, max_text_len=20, dim_text_hidden=512, dim_coemb_hidden=512, dim_pose=self.dim_pose,
                        dim_movement_enc_hidden=512, dim_movement_latent=512, checkpoints_dir=checkpoints_dir, unit_length=4)
