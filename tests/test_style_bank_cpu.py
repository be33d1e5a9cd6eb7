"""Several styles in one batch, without a GPU: the segment planner of the style-aware kernels (mst_plan_style_segments) and the
StyleBank's construction-time checks (csrc/mst_style.h, model/style_bank.py)."""
import numpy as np
import pytest
import torch

import mst_amd  # noqa: F401


def _assignments(n):
    return {
        "interleaved": [(0, 1, 1, 2, 0, 2)[i % 6] for i in range(n)],
        "grouped": sorted(i * 3 // n for i in range(n)),
        "uniform": [1] * n,
        "cycle": [i % 3 for i in range(n)],
        "odd": [1 if i != n // 2 else 2 for i in range(n)],             # a single clip of another style
        "pairs": [(i // 2) % 3 for i in range(n)],                        # runs of two
    }


@pytest.mark.parametrize("S", [18, 33, 41, 77, 197])
@pytest.mark.parametrize("tile_rows", [16, 32, 48, 64])
@pytest.mark.parametrize("nclips", [1, 4, 13, 64])
def test_planner_covers_every_row_once(S, tile_rows, nclips):
    import __graft_entry__ as g
    g.build()
    from mst_amd.engine import plan_style_segments
    M = nclips * S
    tiles = (M + tile_rows - 1) // tile_rows
    for name, styles in _assignments(nclips).items():
        seg = plan_style_segments(styles, S, tile_rows)
        assert len(seg) <= tiles + nclips, name
        seen = np.zeros(M, np.int32)
        for row0, lo, hi, slot in seg:
            assert row0 % tile_rows == 0 and row0 <= lo < hi <= min(row0 + tile_rows, M), (name, row0, lo, hi)
            clips = {r // S for r in range(lo, hi)}
            assert {styles[c] for c in clips} == {slot}, (name, row0, lo, hi)    # no segment mixes two styles
            seen[lo:hi] += 1
        assert (seen == 1).all(), name                                           # every row exactly once
        # maximal runs: two neighbouring segments of one tile have different slots
        for a, b in zip(seg[:-1], seg[1:]):
            if a[0] == b[0]:
                assert a[3] != b[3] and a[2] == b[1], name
        if name == "uniform":
            assert len(seg) == tiles


@pytest.mark.parametrize("nclips", [24, 56])
def test_short_clips_put_several_segments_in_one_tile(nclips):
    """18-token clips (T = 17), styles cycling: 48- and 64-row tiles each hold >= 3 segments somewhere, so that the GPU cases of
    tests/test_gpu_style_kernels.py at T = 17 run several workgroups over one tile."""
    import __graft_entry__ as g
    g.build()
    from mst_amd.engine import plan_style_segments
    styles = _assignments(nclips)["cycle"]
    for tile_rows in (48, 64):
        seg = plan_style_segments(styles, 18, tile_rows)
        per_tile = np.unique(seg[:, 0], return_counts=True)[1]
        assert per_tile.max() >= 3, (tile_rows, per_tile)
    odd = [r for r in plan_style_segments(_assignments(nclips)["odd"], 18, 64) if r[3] == 2]
    c = nclips // 2                                                     # the odd clip: its own segment (two across a tile edge)
    assert 1 <= len(odd) <= 2 and odd[0][1] == 18 * c and odd[-1][2] == 18 * c + 18, odd


def test_planner_reports_a_short_table():
    import ctypes as C
    from mst_amd import _native
    lib = _native.lib()
    styles = np.array([0, 1, 0, 1], np.int32)
    out = np.zeros((2, 4), np.int32)
    n = lib.mst_plan_style_segments(styles.ctypes.data_as(C.c_void_p), 4, 77, 64, out.ctypes.data_as(C.c_void_p), 2)
    assert n == -1
    assert b"segments" in lib.mst_last_error()


def test_null_engine_style_entries_fail_cleanly():
    from mst_amd import _native
    lib = _native.lib()
    assert lib.mst_style_slots(None, 2) != 0
    assert lib.mst_load_layers_slot(None, 1, None, None) != 0
    assert lib.mst_set_styles(None, None, 0, None) != 0


def _style(seed, njoints=24, layers=2, prior_seed=0):
    from mst_amd.model.mdm_forstyledataset import StyleDiffusion
    torch.manual_seed(prior_seed)
    m = StyleDiffusion("", njoints, 1, 1, True, "rot6d", True, True, latent_dim=512, ff_size=1024, num_layers=layers, num_heads=4,
                       dropout=0.1, activation="gelu", data_rep="hml_vec", cond_mode="text", cond_mask_prob=0.1,
                       arch="trans_enc", dataset="stylexia_posrot")
    torch.manual_seed(1000 + seed)
    for p in m.seqTransEncoder.parameters():
        p.data.normal_(0, 0.02)
    return m


def test_bank_rejects_another_prior():
    from mst_amd.model.style_bank import StyleBank
    a, b = _style(0), _style(1)
    StyleBank([a, b])                                                   # same prior, other stacks: fine
    c = _style(2)
    with torch.no_grad():
        c.motion_enc.mdm_model.embed_text.bias.add_(1.0)
    with pytest.raises(ValueError, match="embed_text.bias"):
        StyleBank([a, c])
    with pytest.raises(ValueError, match="num_layers"):
        StyleBank([a, _style(3, layers=1)])
    with pytest.raises(ValueError, match="poseEmbedding.weight"):
        StyleBank([a, _style(4, njoints=25)])


def test_bank_rejects_a_style_index_out_of_range():
    from mst_amd.model.style_bank import StyleBank
    bank = StyleBank([_style(0), _style(1)])
    assert bank.num_styles == 2
    assert bank._styles({}, 3, None).tolist() == [0, 0, 0]
    assert bank._styles({"style": torch.tensor([1, 0, 1])}, 3, None).tolist() == [1, 0, 1]
    with pytest.raises(ValueError, match="style index 2 outside"):
        bank._styles({"style": torch.tensor([0, 2, 1])}, 3, None)
    with pytest.raises(ValueError, match="style index -1 outside"):
        bank._styles({"style": torch.tensor([-1, 0, 1])}, 3, None)
    with pytest.raises(ValueError, match="names 2 clips"):
        bank._styles({"style": torch.tensor([0, 1])}, 3, None)


def test_bank_refuses_autograd_and_training():
    from mst_amd.model.style_bank import StyleBank
    bank = StyleBank([_style(0), _style(1)])
    with pytest.raises(RuntimeError, match="sampling"):
        bank.train()
    x = torch.zeros(1, 24, 1, 20, requires_grad=True)
    with pytest.raises(RuntimeError, match="autograd"):
        bank(x, torch.zeros(1, dtype=torch.long), {})
    from mst_amd.diffusion import gaussian_diffusion as gd
    with pytest.raises(RuntimeError, match="StyleBank"):
        gd._refuse_bank(bank, "p_sample_with_grad")
