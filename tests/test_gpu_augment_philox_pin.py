"""What both samplers draw from Philox for one fixed input, pinned byte for byte (tests/golden/augment_philox_pin.npz, recorded
by tests/golden/make_golden_augment_philox_pin.py).

The tape tests fix the samplers' arithmetic and the other Philox tests check determinism, invariants and rates; the crop
trials that run side by side on a wave's lanes (the shuffled box centres, the lowest passing lane) exist on the Philox path
alone, and only this fixture says what they must give.  The input is test_gpu_augment_pair's _ragged(17, ...): one image more
than the block has waves, one image with 70 truths (more than a wave has lanes) and one with none."""
import os

import numpy as np
import pytest
import torch

import _augment_pair_ref as P
import _augment_ref as R
from tdrn_amd.utils.augmentations import PairSSDAugmentation, SSDAugmentation, pair_params_to_dicts, params_to_dicts
from test_gpu_augment import MEAN, _dev, _rows
from test_gpu_augment_pair import _ragged, _tt

DEV = "cuda:0"
gpu = pytest.mark.gpu
B, S = 17, 33
SEED = 1                                    # of _ragged's input and of the Philox key
IDS = list(range(40, 40 + B))


def _hw(imgs):
    return [im.shape[:2] for im in imgs]


def _pin(params, packed, packed_t=None):
    k = int(packed.offsets[-1])
    d = dict(params=params.cpu().numpy(), offsets=packed.offsets.cpu().numpy(), rows=packed.truths[:k].cpu().numpy())
    if packed_t is not None:
        d["rows_t"] = packed_t.truths[:k].cpu().numpy()
    return d


def sample_single(seed=SEED):
    """-> (the frames, the records, PackedTargets, what the fixture keeps of them)"""
    imgs, targets, _, _ = _ragged(B, seed, False)
    params, packed = SSDAugmentation(S, MEAN, seed=seed).sample(_hw(imgs), _tt(targets), torch.device(DEV), sample_ids=IDS)
    return imgs, params, packed, _pin(params, packed)


def sample_pair(supplied, seed=SEED):
    """-> (frames 0, frames 1 or None, the records, both PackedTargets, what the fixture keeps of them)"""
    imgs, targets, imgs_t, targets_t = _ragged(B, seed, supplied)
    params, packed, packed_t = PairSSDAugmentation(S, MEAN, seed=seed).sample(
        _hw(imgs), _tt(targets), torch.device(DEV), sample_ids=IDS, targets_t=_tt(targets_t) if supplied else None)
    return imgs, imgs_t, params, packed, packed_t, _pin(params, packed, packed_t)


def _assert_pinned(z, prefix, got):
    for k, v in got.items():
        want = z[prefix + k]
        assert v.dtype == want.dtype and v.shape == want.shape, (prefix + k, v.dtype, v.shape, want.dtype, want.shape)
        assert v.tobytes() == want.tobytes(), (prefix + k, np.flatnonzero(v.reshape(-1) != want.reshape(-1))[:8])


@gpu
def test_single_sampler_gives_the_pinned_bytes(golden_dir):
    z = np.load(os.path.join(golden_dir, "augment_philox_pin.npz"))
    assert int(z["seed"]) == SEED
    imgs, params, packed, got = sample_single()
    _assert_pinned(z, "single_", got)
    ps = params_to_dicts(params)
    assert any(p["cropped"] == 1 for p in ps)
    assert ps[9]["kept"] == 0 and got["offsets"][-1] == sum(p["kept"] for p in ps)
    x = SSDAugmentation(S, MEAN).apply(_dev(imgs), params).cpu().numpy()
    for b, p in enumerate(ps):
        want = R.apply(imgs[b], p, S, MEAN, to_rgb=True)
        assert np.array_equal(x[b], want), (b, float((x[b] == want).mean()))
    assert [len(r) for r in _rows(packed)] == [p["kept"] for p in ps]


@gpu
def test_pair_sampler_gives_the_pinned_bytes(golden_dir):
    z = np.load(os.path.join(golden_dir, "augment_philox_pin.npz"))
    assert int(z["seed"]) == SEED
    for supplied, prefix in ((False, "pair_translated_"), (True, "pair_supplied_")):
        imgs, imgs_t, params, packed, packed_t, got = sample_pair(supplied)
        _assert_pinned(z, prefix, got)
        ps = pair_params_to_dicts(params)
        assert any(p["cropped"] == 1 for p in ps), prefix
        if supplied:
            assert all(p["attempts"] == 0 and (p["trans_x"], p["trans_y"]) == (0, 0) for p in ps)
        else:
            assert any(p["attempts"] >= 2 for p in ps) and any(p["trans_x"] or p["trans_y"] for p in ps)
        x, x_t = PairSSDAugmentation(S, MEAN).apply(_dev(imgs), params, _dev(imgs_t) if supplied else None)
        x, x_t = x.cpu().numpy(), x_t.cpu().numpy()
        for b, p in enumerate(ps):
            w0, w1 = P.apply_pair(imgs[b], p, S, MEAN, True, imgs_t[b] if supplied else None)
            assert np.array_equal(x[b], w0), (prefix, b, float((x[b] == w0).mean()))
            assert np.array_equal(x_t[b], w1), (prefix, b, float((x_t[b] == w1).mean()))
