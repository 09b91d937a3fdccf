"""Host side of the duplicate-caption mask (no GPU): the module keyword and its
hparam, the caption keys, the experiment, the synthetic datamodule's caption ids,
and the reference's retired arguments, which keep raising.
"""
import functools
import os
import subprocess
import sys

import pytest
import torch

from tests.conftest import PKG, ROOT


def make(**kw):
    from src.models.pretrain.VisionLanguageModule import VisionLanguageModule
    return VisionLanguageModule("resnet34", "tinybert", functools.partial(torch.optim.AdamW, lr=5e-5),
                                kw.pop("deduplicate", False), kw.pop("masked_loss", False), 512, 312, 128,
                                device="cpu", **kw)


def test_keyword_constructs_and_is_saved():
    m = make(duplicate_caption_mask=True)
    assert m.hparams["duplicate_caption_mask"] is True
    assert make().hparams["duplicate_caption_mask"] is False
    # keys: a carried caption_id tensor wins over the strings; flag off: no keys at all
    batch = {"caption": ["a", "b", "a"], "caption_id": torch.tensor([5, 6, 5])}
    assert torch.equal(m._caption_keys(batch), torch.tensor([5, 6, 5]))
    k = m._caption_keys({"caption": ["a", "b", "a"]})
    assert k.dtype == torch.int64 and k[0] == k[2] and k[0] != k[1]
    assert make()._caption_keys(batch) is None


def test_caption_hash_is_fixed_across_interpreters():
    """BLAKE2b-64 of the UTF-8 bytes: the same in this process, in a fresh interpreter with
    another hash salt, and on every rank (Python's hash() differs between the two)."""
    from vlp_amd.clip_model import caption_hash64, compact_caption_ids
    want = [3405396810240292928, 9129465981389454959]
    caps = ["a", "fracture of the distal radius"]
    assert caption_hash64(caps).tolist() == want
    code = (f"import sys; sys.path[:0] = [{ROOT!r}, {PKG!r}]\n"
            "from vlp_amd.clip_model import caption_hash64\n"
            f"print(caption_hash64({caps!r}).tolist())")
    for salt in ("1", "2"):
        r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, PYTHONHASHSEED=salt),
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        assert r.stdout.strip() == str(want)
    ids = compact_caption_ids(caption_hash64(["a", "b", "a", "c"]))
    assert ids.dtype == torch.int32 and ids.tolist() == [1, 2, 1, 0]     # ranks of the hashes


def test_masked_experiment_composes():
    from src.utils.config import compose
    c = compose("train", ["experiment=pretrain/pretrain_resnet34_tinybert_mi355x_masked"])
    base = compose("train", ["experiment=pretrain/pretrain_resnet34_tinybert_mi355x"])
    assert c["model"]["duplicate_caption_mask"] is True and c["data"]["n_unique_captions"] == 880
    assert "duplicate_caption_mask" not in base["model"] and "n_unique_captions" not in base["data"]
    for k in ("batch_size", "image_size", "n_samples"):
        assert c["data"][k] == base["data"][k]
    assert c["model"]["compute_dtype"] == "bf16" and c["model"]["masked_loss"] is False


def test_datamodule_caption_ids_follow_captions():
    from src.data.PretrainDataModule import PretrainDataModule
    dm = PretrainDataModule(batch_size=8, num_workers=0, image_size=32, n_samples=16, n_val_samples=8,
                            seq_len=12, n_unique_captions=3)
    b = next(iter(dm.train_dataloader()))
    cid, cap = b["caption_id"], b["caption"]
    assert cid.dtype == torch.int64 and cid.shape == (8,)
    assert len(set(cap)) <= 3 and len(set(cid.tolist())) == len(set(cap))
    tok = b["caption_tokenized"]["input_ids"]
    for i in range(8):
        for j in range(8):
            same = cid[i].item() == cid[j].item()
            assert same == (cap[i] == cap[j]) and same == torch.equal(tok[i], tok[j])
    # the default keeps one caption per sample, with the samples it drew before the knob existed
    d0 = PretrainDataModule(batch_size=8, num_workers=0, image_size=32, n_samples=16, n_val_samples=8, seq_len=12)
    s = d0.train_dataset[5]
    assert s["caption"].endswith(" radiograph 5")
    assert len({d0.train_dataset[i]["caption_id"] for i in range(16)}) == 16
    s3 = dm.train_dataset[5]
    assert torch.equal(s3["x-ray-u8"], s["x-ray-u8"]) and s3["label"] == s["label"]   # only the caption moved
    assert s3["caption"].endswith(" radiograph 2")


def test_retired_arguments_still_raise():
    from tests.golden.synth import synth_batch
    batch = synth_batch(2, 32, 12, 0)
    m = make(masked_loss=True, duplicate_caption_mask=True)
    with pytest.raises(DeprecationWarning):
        m.training_step(batch)
    with pytest.raises(DeprecationWarning):
        m._compute_loss(torch.zeros(2, 2), False, True, None, torch.tensor([0, 0]))
    with pytest.raises(DeprecationWarning):
        m._compute_loss(torch.zeros(2, 2))            # deduplicate defaults to True, as in the reference
