#!/usr/bin/env python
"""End-to-end on one MI355X through the library's token input pipeline (``device_tokens: True``): synthetic, already-tokenised sentences (a class
prefers its own slice of the vocabulary; four lengths, or every length from 2 to max_length with ``--lengths free``), a tiny BERT or BERT-base, SRSoftMatch or SRPseudoLabel.  The rows go in
as a plain ``dataset_dict``; the engine packs them into one flat int32 store on the device, builds the reference's sampler stream, and every view
of a batch -- gather, right-padding to the batch's longest row, the lengths -- is one launch (data/device_tokens.py, csrc/token_view.hip).
``alg.train()`` / ``alg.evaluate()`` run with no hand-written batch generator and no tokenizer in the step.

SRSoftMatch takes a strong view: the unlabelled set carries two variants of every sentence (``data_s``), here a stand-in for the reference's
back-translations (tokens dropped and swapped).  With strings instead of token arrays the sentences are tokenised once, at construction, by the
tokenizer of the net's snapshot directory (``pretrain_path`` or the hub cache; configs/README.md).  With ``--device-strong``
(``device_tokens_strong: True``) there is no ``data_s``: the loader makes every strong view on the device from the clean sentence -- two
token-level slots (delete / mask / cutoff / swap) drawn per sample and epoch, one launch (csrc/token_strong.hip) -- and a strong-view algorithm
trains on sentences that have no back-translations.

    python examples/train_device_tokens.py --steps 60
    python examples/train_device_tokens.py --steps 60 --algorithm srpseudolabel
    python examples/train_device_tokens.py --steps 60 --run-hooks     # the reference's evaluation / checkpoint / logging hooks drive the run
    python examples/train_device_tokens.py --steps 20 --net base      # BERT-base (random init unless a snapshot is on disk), max_length 128
    python examples/train_device_tokens.py --steps 60 --device-strong # SRFlexMatch, strong views made on the device, no data_s
    python examples/train_device_tokens.py --steps 60 --lengths free  # rows of every length 2 .. max_length: the engine's memory follows the largest batch
    python examples/train_device_tokens.py --steps 60 --lengths free --bucket 16      # token_len_bucket: padded lengths in multiples of 16
"""
import argparse
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from semireward_amd.algorithms import get_algorithm          # noqa: E402
from semireward_amd.core.hooks import Hook                   # noqa: E402
from semireward_amd.nets import bert                         # noqa: E402

CLS, SEP, FIRST = 2, 3, 5                                     # [CLS], [SEP], the first ordinary id of the synthetic vocabulary (4: its [MASK])
# 'lengths': the four row lengths of the default; --lengths free draws every row's length from 2 .. max(lengths) (real text: hundreds of
# distinct padded lengths; the engine's workspaces are sized by the largest batch, configs/README.md)
NETS = {"tiny": dict(builder=bert.bert_tiny_test, vocab=120, lengths=(8, 16, 24, 32), feature_dim=128, lr=5e-4, mask_id=4),
        "base": dict(builder=bert.bert_base_uncased, vocab=30522, lengths=(32, 64, 96, 128), feature_dim=768, lr=5e-5, mask_id=103)}


def synth_rows(n, num_classes, vocab, lengths, seed):
    """n int32 rows [CLS] w ... [SEP] of one of ``lengths`` tokens (a range: of any length in it): 70 % of the words come from the class's slice
    of the vocabulary; + labels."""
    rng = np.random.Generator(np.random.PCG64(seed))
    y = rng.integers(0, num_classes, size=n)
    width = (vocab - FIRST) // num_classes
    out = []
    for c in y:
        m = int(lengths[rng.integers(0, len(lengths))]) - 2
        own = FIRST + c * width + rng.integers(0, width, size=m)
        w = np.where(rng.random(m) < 0.7, own, rng.integers(FIRST, vocab, size=m))
        out.append(np.concatenate([[CLS], w, [SEP]]).astype(np.int32))
    return out, y.astype(np.int64)


def variant(row, rng):
    """A stand-in for a back-translation: every fifth word dropped on average, one pair of neighbours swapped (the length changes: rows of a
    strong batch are padded to their own longest)."""
    w = row[1:-1]
    w = w[rng.random(w.size) > 0.2]
    if w.size > 2:
        i = int(rng.integers(0, w.size - 1))
        w[[i, i + 1]] = w[[i + 1, i]]
    return np.concatenate([[CLS], w, [SEP]]).astype(np.int32)


class PrintHook(Hook):
    def after_train_step(self, alg):
        if alg.it % 10 == 0 or alg.it == alg.num_train_iter - 1:
            print("it %3d  epoch %d  sup %.3f  unsup %.3f  util %.2f" % (alg.it, alg.epoch, float(alg.log_dict["train/sup_loss"]),
                                                                        float(alg.log_dict["train/unsup_loss"]),
                                                                        float(alg.log_dict["train/util_ratio"])), flush=True)


ALGORITHMS = {"srpseudolabel": dict(unsup_warm_up=0.4, p_cutoff=0.95),
              "srsoftmatch": dict(dist_align=True, dist_uniform=True, per_class=False, ema_p=0.999, n_sigma=2),
              "srflexmatch": dict(thresh_warmup=True, p_cutoff=0.95)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--classes", type=int, default=4)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--net", choices=sorted(NETS), default="tiny")
    ap.add_argument("--algorithm", choices=sorted(ALGORITHMS), default=None, help="srsoftmatch; srflexmatch with --device-strong")
    ap.add_argument("--device-strong", action="store_true",
                    help="device_tokens_strong: the strong views are made on the device from the clean sentences, no data_s")
    ap.add_argument("--lengths", choices=("four", "free"), default="four",
                    help="free: every row's length is drawn from the whole 2 .. max_length range instead of four values")
    ap.add_argument("--bucket", type=int, default=None, help="token_len_bucket: padded lengths are rounded up to multiples of this")
    ap.add_argument("--run-hooks", action="store_true",
                    help="run_hooks + device_eval: evaluate and checkpoint every steps / 2 steps (into a temporary save_dir), log every 10")
    a = ap.parse_args()
    a.algorithm = a.algorithm or ("srflexmatch" if a.device_strong else "srsoftmatch")
    C, net = a.classes, NETS[a.net]
    lengths = range(2, max(net["lengths"]) + 1) if a.lengths == "free" else net["lengths"]
    x_lb, y_lb = synth_rows(10 * C, C, net["vocab"], lengths, 1)
    x_ulb, _ = synth_rows(512, C, net["vocab"], lengths, 2)
    x_te, y_te = synth_rows(128, C, net["vocab"], lengths, 3)
    ulb = {"data": x_ulb, "targets": None}
    if a.algorithm != "srpseudolabel" and not a.device_strong:   # its train_step takes x_ulb_s: two variants per sentence
        rng = np.random.Generator(np.random.PCG64(4))
        ulb["data_s"] = [[variant(r, rng) for r in x_ulb] for _ in range(2)]
    steps = max(a.steps, a.epochs) // a.epochs * a.epochs
    args = argparse.Namespace(
        algorithm=a.algorithm, num_classes=C, num_train_iter=steps, epoch=a.epochs, ema_m=0.0, ulb_loss_ratio=1.0, use_cat=False, amp=False,
        lr=net["lr"], weight_decay=5e-4, layer_decay=0.75, num_warmup_iter=5, optim="AdamW", T=0.5, hard_label=True, N_k=10, start_timing=20,
        feature_dim=net["feature_dim"], sr_lr=5e-4, sr_ema=False, sr_ema_m=0.99, gpu=0, rank=0, world_size=1, distributed=False, seed=0,
        # the input pipeline: what a usb_nlp yaml says (max_length, batch sizes, sampler) + the rows + the option
        dataset="synthetic_tokens", max_length=max(net["lengths"]), batch_size=a.batch, uratio=1, eval_batch_size=16,
        train_sampler="RandomSampler", device_tokens=True, device_tokens_strong=a.device_strong, device_tokens_mask_id=net["mask_id"],
        dataset_dict={"train_lb": {"data": x_lb, "targets": y_lb}, "train_ulb": ulb, "eval": {"data": x_te, "targets": y_te}},
        **({} if a.bucket is None else dict(token_len_bucket=a.bucket)), **ALGORITHMS[a.algorithm])
    if a.run_hooks:
        with tempfile.TemporaryDirectory() as save_dir:
            vars(args).update(run_hooks=True, device_eval=True, num_eval_iter=max(steps // 2, 1), num_log_iter=10, save_dir=save_dir,
                              save_name="example")
            alg = get_algorithm(args, net["builder"])
            alg.train()
            print("results:", alg.results_dict, " files:", sorted(os.listdir(os.path.join(save_dir, "example"))))
            ev = alg.evaluate("eval")
    else:
        alg = get_algorithm(args, net["builder"])
        alg.register_hook(PrintHook(), "PrintHook", "LOWEST")
        alg.train()
        ev = alg.evaluate("eval")
    print("eval:", {k: round(float(v), 4) for k, v in ev.items()})
    return ev


if __name__ == "__main__":
    main()
