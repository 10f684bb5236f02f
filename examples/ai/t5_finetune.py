#!/usr/bin/env python3
"""Fine-tune T5 from a local checkpoint directory or from random init.

    python examples/ai/t5_finetune.py                                   # t5-small topology, synthetic copy task
    python examples/ai/t5_finetune.py --size tiny --max-steps 40 --lr 3e-3 --eval-generate 2
    python examples/ai/t5_finetune.py --checkpoint /models/t5-small --data pairs.jsonl --epochs 3
    python examples/ai/t5_finetune.py --checkpoint /models/t5-small --text-file en_de.tsv --eval-generate 4
    python examples/ai/t5_finetune.py --checkpoint /models/flan-t5-base --text-file qa.tsv
    cloudtik-run --nproc 8 examples/ai/t5_finetune.py --size base --batch 16

The other half of the reference's T5 entry (HF ``run_translation.py --do_train``).  d_kv-64
topologies (t5-small, t5-base, t5-large) and d_kv-128 ones (a t5-3b / t5-11b checkpoint, or ``--d-kv 128``) train end to end on the MFMA attention kernels: the
relative-position bias is added inside the kernel, whose backward also returns the gradient of the
bias vector, and both self- and cross-attention take dropout there.  ``CLOUDTIK_AMD_T5_TRAIN_ATTN=0``
sends those calls to ``F.scaled_dot_product_attention`` instead.  T5 v1.1 / Flan-T5 checkpoints (and
``--size v1.1-small`` .. ``v1.1-xxl``) train their untied head and run the gated-GELU feed-forward with its
dropout as one kernel forward and one backward (``CLOUDTIK_AMD_T5_FUSED_FF=0``: the PyTorch composition).

Training pairs, in this order of preference:

* ``--data FILE``: JSON lines of ``{"input_ids": [...], "labels": [...]}`` (token ids).
* ``--text-file FILE``: lines of ``source<TAB>target``, tokenized with the checkpoint's
  ``spiece.model`` (needs ``--checkpoint`` and the ``transformers`` tokenizer; nothing is downloaded).
* otherwise a seeded synthetic copy task: random sources, the target is the source followed by EOS.

Batches are padded to their longest source and target, with ``attention_mask`` and ``-100`` labels.
``--checkpoint`` is a directory holding ``config.json`` and ``model.safetensors``, ``pytorch_model.bin`` or
a sharded checkpoint with its index (``T5ForConditionalGeneration.from_pretrained``); ``--size`` selects a random-init topology (``--d-kv`` / ``--dropout`` override
it).  Trains through ``cloudtik_amd.train.trainer.Trainer`` with the fused AdamW, prints the loss
every ``--log-every`` steps and one JSON result line, and with ``--eval-generate N`` prints greedy
outputs for N sources at the end.
"""
import argparse
import json
import logging
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

import torch  # noqa: E402


_V1_1 = ["v1.1-small", "v1.1-base", "v1.1-large", "v1.1-xl", "v1.1-xxl"]


def load_model(checkpoint, size, device, dtype, d_kv=None, dropout=None):
    from cloudtik_amd.models.t5 import T5Config, T5ForConditionalGeneration
    if checkpoint is None:
        kw = {}
        if d_kv is not None:
            kw["d_kv"] = d_kv
        if dropout is not None:
            kw["dropout_rate"] = dropout
        cfg = T5Config.v1_1(size[len("v1.1-"):], **kw) if size.startswith("v1.1-") else getattr(T5Config, size)(**kw)
        return T5ForConditionalGeneration(cfg, device=device, dtype=dtype)
    model = T5ForConditionalGeneration.from_pretrained(checkpoint, device=device, dtype=dtype)
    if dropout is not None:
        model.cfg.dropout_rate = dropout
    return model


def load_tokenizer(checkpoint):
    if checkpoint is None or not os.path.exists(os.path.join(checkpoint, "spiece.model")):
        return None
    try:
        from transformers import AutoTokenizer
        return AutoTokenizer.from_pretrained(checkpoint, local_files_only=True)
    except Exception as e:  # noqa: BLE001 - the example still runs on token ids
        print(f"no tokenizer ({e})")
        return None


def load_pairs(a, cfg, tok):
    """A list of (input_ids, labels) lists of token ids."""
    if a.data:
        with open(a.data) as f:
            rows = [json.loads(line) for line in f if line.strip()]
        return [(r["input_ids"], r["labels"]) for r in rows]
    if a.text_file:
        if tok is None:
            raise SystemExit("--text-file needs --checkpoint with a spiece.model and the transformers tokenizer")
        pairs = []
        with open(a.text_file) as f:
            for line in f:
                if "\t" in line:
                    src, tgt = line.rstrip("\n").split("\t", 1)
                    pairs.append((tok(src, truncation=True, max_length=a.max_source_len)["input_ids"],
                                  tok(tgt, truncation=True, max_length=a.max_target_len)["input_ids"]))
        return pairs
    g = torch.Generator().manual_seed(a.seed)
    pairs = []
    for _ in range(a.synthetic_pairs):
        n = int(torch.randint(max(1, a.source_len // 2), a.source_len + 1, (1,), generator=g))
        src = torch.randint(2, cfg.vocab_size, (n,), generator=g).tolist()
        pairs.append((src, src + [cfg.eos_token_id]))
    return pairs


class PairLoader:
    """Batches of pairs padded to the batch maximum; reshuffled per epoch from the seed, and each
    rank takes its stride of the batches."""

    def __init__(self, pairs, batch, pad_id, seed, rank=0, world=1):
        self.pairs, self.batch, self.pad_id, self.seed = pairs, batch, pad_id, seed
        self.rank, self.world, self.epoch = rank, world, 0

    def set_epoch(self, epoch):
        self.epoch = epoch

    def __len__(self):
        return len(self.pairs) // (self.batch * self.world)

    def collate(self, rows):
        ls, lt = max(len(s) for s, _ in rows), max(len(t) for _, t in rows)
        ids = torch.full((len(rows), ls), self.pad_id, dtype=torch.long)
        mask = torch.zeros(len(rows), ls, dtype=torch.long)
        labels = torch.full((len(rows), lt), -100, dtype=torch.long)
        for i, (s, t) in enumerate(rows):
            ids[i, :len(s)] = torch.tensor(s)
            mask[i, :len(s)] = 1
            labels[i, :len(t)] = torch.tensor(t)
        return {"input_ids": ids, "attention_mask": mask, "labels": labels}

    def __iter__(self):
        g = torch.Generator().manual_seed(self.seed + self.epoch)
        order = torch.randperm(len(self.pairs), generator=g).tolist()
        for n in range(len(self)):
            start = (n * self.world + self.rank) * self.batch
            yield self.collate([self.pairs[i] for i in order[start:start + self.batch]])


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--checkpoint", default=None, help="local directory with config.json and the weights")
    ap.add_argument("--size", default="small", choices=["tiny", "small", "base", "large"] + _V1_1, help="random-init topology")
    ap.add_argument("--d-kv", type=int, default=None, help="override the topology's head dim (random init)")
    ap.add_argument("--dropout", type=float, default=None, help="override the dropout rate")
    ap.add_argument("--data", default=None, help='JSON lines of {"input_ids": [...], "labels": [...]}')
    ap.add_argument("--text-file", default=None, help="lines of source<TAB>target (needs the tokenizer)")
    ap.add_argument("--max-source-len", type=int, default=512)
    ap.add_argument("--max-target-len", type=int, default=128)
    ap.add_argument("--synthetic-pairs", type=int, default=2048, help="size of the synthetic copy task")
    ap.add_argument("--source-len", type=int, default=24, help="longest synthetic source")
    ap.add_argument("--batch", type=int, default=16, help="pairs per step and rank")
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--weight-decay", type=float, default=0.0)
    ap.add_argument("--epochs", type=int, default=1)
    ap.add_argument("--max-steps", type=int, default=0, help="stop after this many optimizer steps (0: off)")
    ap.add_argument("--grad-accum", type=int, default=1)
    ap.add_argument("--clip-norm", type=float, default=1.0, help="0: off")
    ap.add_argument("--checkpoint-dir", default=None, help="save (and resume) training state here")
    ap.add_argument("--log-every", type=int, default=10)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--eval-generate", type=int, default=0, metavar="N", help="greedy outputs for N sources at the end")
    a = ap.parse_args(argv)

    logging.basicConfig(level=logging.INFO, format="%(message)s", stream=sys.stdout)
    from cloudtik_amd import ops
    from cloudtik_amd.train.trainer import Trainer, setup_distributed

    rank, world, device = setup_distributed()
    torch.manual_seed(a.seed)
    ops.manual_seed(a.seed + rank)
    dtype = torch.bfloat16 if device.type == "cuda" else torch.float32
    model = load_model(a.checkpoint, a.size, device, dtype, a.d_kv, a.dropout)
    tok = load_tokenizer(a.checkpoint)
    pairs = load_pairs(a, model.cfg, tok)
    if len(pairs) < a.batch * world:
        raise SystemExit(f"{len(pairs)} training pairs are fewer than one batch per rank")
    loader = PairLoader(pairs, a.batch, model.cfg.pad_token_id, a.seed, rank, world)

    losses = []

    def step(m, b):
        loss = m(b["input_ids"], b["labels"], b["attention_mask"])
        losses.append(loss.detach())
        return loss, {"loss": loss.detach()}

    trainer = Trainer(model, optimizer="adamw", lr=a.lr, weight_decay=a.weight_decay, train_loader=loader, step_fn=step,
                      epochs=a.epochs, max_steps=a.max_steps or None, grad_accum=a.grad_accum,
                      clip_norm=a.clip_norm or None, checkpoint_dir=a.checkpoint_dir, log_every=a.log_every)
    trainer.fit()
    n = max(1, min(5, len(losses) // 2))
    result = {"steps": trainer.global_step, "pairs": len(pairs), "world": world,
              "first_loss": round(float(torch.stack(losses[:n]).float().mean()), 4) if losses else None,
              "final_loss": round(float(torch.stack(losses[-n:]).float().mean()), 4) if losses else None}
    if a.eval_generate and rank == 0:
        model.eval()
        batch = loader.collate(pairs[:a.eval_generate])
        out = model.generate(batch["input_ids"].to(device), batch["attention_mask"].to(device),
                             max_new_tokens=min(a.max_target_len, max(len(t) for _, t in pairs[:a.eval_generate]) + 1))
        show = (lambda row: tok.decode(row, skip_special_tokens=True)) if tok is not None else (lambda row: list(row))
        for i, (src, tgt) in enumerate(pairs[:a.eval_generate]):
            print(f"[{i}] source: {show(src)}")
            print(f"[{i}] target: {show(tgt)}")
            print(f"[{i}] greedy: {show(out[i].tolist())}")
    trainer.close()
    if rank == 0:
        print(json.dumps(result), flush=True)
    return result


if __name__ == "__main__":
    main()
