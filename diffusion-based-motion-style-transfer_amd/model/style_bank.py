"""Several fine-tuned styles sampled in one batch.

Each style is its own fine-tuned `StyleDiffusion`; two of them differ only in the 96 tensors of `seqTransEncoder.layers.*` -- the pose
embedding, output projection, timestep MLP, text projection and positional table all come from the frozen `motion_enc.mdm_model`
(reference model/mdm_forstyledataset.py:602-625, :84-85).  The reference demo samples one style model at a time
(sample/demo_style_transfer.py:74-85, 244-258).  A `StyleBank` holds K such models in ONE native engine (style slots, csrc/mst_style.h)
and picks the stack per clip: `model_kwargs['y']['style']` is a LongTensor[bs] of indices into the bank (any order; missing = style 0).
Every sampler that accepts a `StyleDiffusion` accepts a bank, `ClassifierFreeSampleModel(bank)` included.  Sampling only: a bank
refuses autograd (the `*_with_grad` samplers, the training node) -- fine-tuning stays per style."""
import torch
import torch.nn as nn

from .native_stack import stack_parameters

_PRIOR_SKIP = ("clip_model.", "seqTransEncoder.")


class StyleBank(nn.Module):
    is_style_bank = True

    def __init__(self, models):
        super().__init__()
        models = list(models)
        if not models:
            raise ValueError("StyleBank needs at least one StyleDiffusion")
        ref = models[0]
        ref_prior = self._prior_tensors(ref)
        for i, m in enumerate(models[1:], 1):
            if m.num_layers != ref.num_layers:
                raise ValueError(f"StyleBank: member {i} has num_layers {m.num_layers}, member 0 has {ref.num_layers}")
            prior = self._prior_tensors(m)
            for name, t in ref_prior.items():
                u = prior.get(name)
                if u is None or u.shape != t.shape or not torch.equal(u.detach().cpu(), t.detach().cpu()):
                    raise ValueError(f"StyleBank: member {i} has another frozen prior than member 0: "
                                     f"motion_enc.mdm_model.{name} differs")
            extra = sorted(set(prior) - set(ref_prior))
            if extra:
                raise ValueError(f"StyleBank: member {i} has another frozen prior than member 0: motion_enc.mdm_model.{extra[0]} differs")
        self.members = nn.ModuleList(models)
        for k in ("input_feats", "num_layers", "latent_dim", "num_heads", "ff_size", "clip_dim", "cond_mask_prob", "cond_mode",
                  "translation", "njoints", "nfeats", "data_rep", "dataset"):
            setattr(self, k, getattr(ref, k))
        self.rot2xyz = getattr(ref, "rot2xyz", None)
        self.train(False)

    @staticmethod
    def _prior_tensors(m):
        return {k: v for k, v in m._prior().state_dict().items() if not k.startswith(_PRIOR_SKIP)}

    @property
    def num_styles(self):
        return len(self.members)

    def train(self, mode=True):
        if mode:
            raise RuntimeError("StyleBank is for sampling; fine-tune each StyleDiffusion on its own")
        return super().train(False)

    # ---- engine plumbing (the _EngineHost role: model/mdm_forstyledataset.py)
    def mst_engine(self, rows, frames):
        """One engine for the whole bank: member 0's weights in slot 0 (kept current by member 0's own parameter-version watch), member
        i's stack in slot i, uploaded again when -- and only when -- that member's stack tensors change."""
        eng = self.members[0].mst_engine(rows, frames, slot="style_bank")
        K = len(self.members)
        if K == 1:
            return eng
        state = self.__dict__.setdefault("_mst_bank", {})
        if state.get("eng") is not eng:                  # a new (larger) engine: its slots start empty
            eng.style_slots(K)
            state.clear()
            state["eng"] = eng
        for i in range(1, K):
            params = stack_parameters(self.members[i].seqTransEncoder)
            # (the member's epoch: its `mst_weights_changed()` count -- writes through `.data` move neither version nor pointer)
            version = (self.members[i].__dict__.get("_mst_epoch", 0),) + tuple(p._version for p in params) + tuple(p.data_ptr() for p in params)
            if state.get(i) != version:
                eng.load_layers_slot(i, [p.detach().float().contiguous() for p in params])
                state[i] = version
        return eng

    def mst_weights_changed(self):
        """Every member's `mst_weights_changed()`: after a write through `.data` (invisible to the version watch) the bank's engine
        uploads slot 0 in full and every other slot's stack again at its next call."""
        for m in self.members:
            m.mst_weights_changed()

    def __deepcopy__(self, memo):
        from .mdm_forstyledataset import _deepcopy_without_engines
        return _deepcopy_without_engines(self, memo)

    def _styles(self, y, bs, device):
        st = None if y is None else y.get('style')
        if st is None:
            return torch.zeros(bs, dtype=torch.long)
        st = torch.as_tensor(st).reshape(-1).to("cpu", torch.long)
        if st.numel() != bs:
            raise ValueError(f"StyleBank: y['style'] names {st.numel()} clips, the batch has {bs}")
        if st.numel() and (int(st.min()) < 0 or int(st.max()) >= len(self.members)):
            bad = int(st[(st < 0) | (st >= len(self.members))][0])
            raise ValueError(f"StyleBank: style index {bad} outside [0, {len(self.members)})")
        return st

    def mst_prepare(self, eng, y, cfg):
        """Text conditioning as a StyleDiffusion uploads it (the prior is shared), plus the slot of every clip."""
        self.members[0].mst_prepare(eng, y, cfg)
        st = self._styles(y, eng.text_rows, eng.device)
        if len(self.members) > 1:
            eng.set_styles(st)

    def _wants_autograd(self, x):
        return torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters()))

    def forward(self, x, timesteps, y=None):
        if self._wants_autograd(x):
            raise RuntimeError("StyleBank: no autograd through a bank (the *_with_grad samplers, the training node); "
                               "fine-tune each StyleDiffusion on its own, or sample under torch.no_grad()")
        eng = self.mst_engine(x.shape[0], x.shape[-1])
        self.mst_prepare(eng, y if y is not None else {}, False)
        return eng.forward(x, timesteps)
