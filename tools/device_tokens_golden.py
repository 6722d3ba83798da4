"""Write tests/golden/device_tokens.npz: what the token store and its loaders (semireward_amd/data/device_tokens.py) are pinned to.

TEST INFRASTRUCTURE (build container only, like tools/device_audio_golden.py): needs transformers and the reference tree, runs on the CPU; the
tests and everything that runs on the GPU machine read only the fixture.  Arrays only (the sentences are rebuilt from their seeds by
tests/_token_view_cases.py; the tiny vocabulary is written to a temporary directory and loaded with BertTokenizerFast.from_pretrained):

  * meta/transformers: the version that tokenised;
  * tok/<max_length>/<split>/flat, len: the ids ``tokenizer(text, max_length=max_length, truncation=True, padding=False)['input_ids']`` of every
    sentence, then of every aug_0, then of every aug_1 (evaluation: the sentences only), for max_length 16 and 64 -- the call of the
    reference's collator (semilearn/datasets/collactors/nlp_collactor.py:51-60);
  * col/e<epoch>/<lb|ulb>/<step>/...: what the reference's own DataCollatorWithPadding (loaded by path) returns for the labelled and
    unlabelled batches of two epochs of the test configuration's index stream, fed with the samples the reference's BasicDataset yields
    ({'idx', 'text', 'label'} / {'idx', 'text', 'text_s'}): idx, y_lb, input_ids, attention_mask and, for the unlabelled batches,
    variant (which of the two augmentations was 'text_s': the loader's own seeded draw, the reference's is an unseeded random.randint) and
    s_input_ids / s_attention_mask;
  * col/eval/<batch>/...: the same for the evaluation set in order, last partial batch kept.

What is independent of the code under test and what is not: input_ids, attention_mask (hence the tokenisation, the truncation and the padding
rule) and the pass-through of idx / label come from the reference's collator and transformers.  WHICH sentences form a batch (idx) and which
variant is 'text_s' (variant) are produced by the loaders under test themselves (``_epoch_table`` / ``draws``): for those two arrays the
fixture is a regression pin, not a comparison with the reference.  That the index stream is the reference's rests on EpochSampler's own test
against the reference's DistributedSampler (tests/test_cpu_device_loader.py, tests/golden/device_data.npz).

    PYTHONDONTWRITEBYTECODE=1 python tools/device_tokens_golden.py
"""
import importlib.util
import os
import sys
import tempfile

import numpy as np
import transformers
from transformers import BertTokenizerFast

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _token_view_cases as TC  # noqa: E402
from oracle import _ref_import as R  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "device_tokens.npz")


def reference_collator(tokenizer, max_length):
    sys.dont_write_bytecode = True
    spec = importlib.util.spec_from_file_location("_ref_nlp_collactor", os.path.join(R.REF, "semilearn", "datasets", "collactors", "nlp_collactor.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m.DataCollatorWithPadding(tokenizer, max_length=max_length)


def np64(t):
    return np.asarray(t.numpy() if hasattr(t, "numpy") else t, dtype=np.int64)


def main():
    out = {"meta/transformers": np.array(transformers.__version__)}
    with tempfile.TemporaryDirectory() as d:
        tokenizer = BertTokenizerFast.from_pretrained(TC.write_vocab_dir(d), local_files_only=True)
    assert tokenizer.vocab_size == len(TC.VOCAB) and tokenizer.pad_token_id == TC.PAD
    for ml in TC.MAX_LENGTHS:
        for split in TC.SPLITS:
            tri = TC.sentences(split)
            texts = [t[0] for t in tri] + ([t[1] for t in tri] + [t[2] for t in tri] if split != "eval" else [])
            rows = [tokenizer(s, max_length=ml, truncation=True, padding=False)["input_ids"] for s in texts]
            out["tok/%d/%s/flat" % (ml, split)] = np.concatenate(rows).astype(np.int32)
            out["tok/%d/%s/len" % (ml, split)] = np.array([len(r) for r in rows], dtype=np.int32)
    c = TC.LOADER
    collate = reference_collator(tokenizer, c["max_length"])
    # the loaders' own index stream and variant draws (host side only: no launch); the collator pads what the reference's dataset would yield
    g = {k: out[k] for k in out}
    dd = TC.loader_dataset_dict(g)
    lb, ulb = TC.loader_pair(dd, "cpu")
    tri_lb, tri_ulb, y = TC.sentences("train_lb"), TC.sentences("train_ulb"), TC.targets("train_lb")
    for epoch in range(c["epoch"]):
        for ld in (lb, ulb):
            ld.set_epoch(epoch)
        tl, _, _ = lb._epoch_table()
        tu, _, _ = ulb._epoch_table()
        for t in range(len(lb)):
            idx = tl[0, t * lb.batch_size:(t + 1) * lb.batch_size]
            b = collate([{"idx": int(i), "text": tri_lb[i][0], "label": int(y[i])} for i in idx])
            p = "col/e%d/lb/%d/" % (epoch, t)
            out[p + "idx"], out[p + "y_lb"] = np64(b["idx_lb"]), np64(b["y_lb"])
            out[p + "input_ids"], out[p + "attention_mask"] = np64(b["x_lb"]["input_ids"]), np64(b["x_lb"]["attention_mask"])
            idx = tu[0, t * ulb.batch_size:(t + 1) * ulb.batch_size]
            src = ulb.draws["x_ulb_s"][0][t * ulb.batch_size:(t + 1) * ulb.batch_size]
            var = src // len(ulb.dataset) - 1
            assert np.array_equal(src % len(ulb.dataset), idx) and set(var.tolist()) <= {0, 1}
            b = collate([{"idx": int(i), "text": tri_ulb[i][0], "text_s": tri_ulb[i][1 + int(v)]} for i, v in zip(idx, var)])
            p = "col/e%d/ulb/%d/" % (epoch, t)
            out[p + "idx"], out[p + "variant"] = np64(b["idx_ulb"]), var.astype(np.int64)
            out[p + "input_ids"], out[p + "attention_mask"] = np64(b["x_ulb_w"]["input_ids"]), np64(b["x_ulb_w"]["attention_mask"])
            out[p + "s_input_ids"], out[p + "s_attention_mask"] = np64(b["x_ulb_s"]["input_ids"]), np64(b["x_ulb_s"]["attention_mask"])
    tri_ev, y_ev = TC.sentences("eval"), TC.targets("eval")
    for t, s in enumerate(range(0, len(tri_ev), c["eval_batch_size"])):
        idx = range(s, min(s + c["eval_batch_size"], len(tri_ev)))
        b = collate([{"idx": i, "text": tri_ev[i][0], "label": int(y_ev[i])} for i in idx])
        p = "col/eval/%d/" % t
        out[p + "y_lb"], out[p + "input_ids"], out[p + "attention_mask"] = np64(b["y_lb"]), np64(b["x_lb"]["input_ids"]), np64(b["x_lb"]["attention_mask"])
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes;", len(out), "arrays")
    lens = out["tok/16/train_ulb/len"]
    print("train_ulb lengths at 16:", lens.tolist())


if __name__ == "__main__":
    main()
