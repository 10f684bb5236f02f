#!/usr/bin/env python3
"""Greedy, beam-search and sampled generation with T5, from a local checkpoint directory or random init.

    python examples/ai/t5_generate.py                                   # t5-small topology, random weights
    python examples/ai/t5_generate.py --checkpoint /models/t5-small --text "translate English to German: Hello"
    python examples/ai/t5_generate.py --num-beams 4 --length-penalty 0.6 --early-stopping
    python examples/ai/t5_generate.py --do-sample --top-k 50 --top-p 0.95 --temperature 0.8 --num-return-sequences 3 --seed 7
    python examples/ai/t5_generate.py --no-repeat-ngram-size 3 --min-length 8 --bad-words 5 --bad-words 17,42
    python examples/ai/t5_generate.py --checkpoint /models/t5-small --task summarization --text "..."
    python examples/ai/t5_generate.py --precision int8                  # every linear and the head in int8
    python examples/ai/t5_generate.py --checkpoint /models/flan-t5-base --text "Answer: is water wet?"
    python examples/ai/t5_generate.py --size v1.1-base                  # T5 v1.1 / Flan-T5 topology, random weights

``--task`` takes the generation settings the checkpoint's ``config.json`` ships for that task
(``task_specific_params``: beams, length penalty, minimum length, n-gram ban, ...) and puts the
task's prefix in front of every ``--text``; flags given on the command line are overridden by it.

``--precision int8`` quantizes the loaded model (``T5ForConditionalGeneration.quantize_dynamic``:
int8 weights with one scale per output channel, activations quantized per token on every call)
and generates with that; every mode and flag works as on the bf16 model.

``--checkpoint`` is a directory holding ``config.json`` and ``model.safetensors``, ``pytorch_model.bin``
or a sharded checkpoint with its index (``T5ForConditionalGeneration.from_pretrained``; nothing is
downloaded): T5 v1.0, or T5 v1.1 / Flan-T5 with the gated-GELU feed-forward and an untied head.  With a ``spiece.model`` in it and the
``transformers`` tokenizer installed, ``--text`` is tokenized and the output decoded; otherwise
random token ids go in and token ids are printed.  Runs on the GPU when there is one.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

import torch  # noqa: E402


_SIZES = {"3b": "xl", "11b": "xxl"}         # --size name -> T5Config constructor
_V1_1 = ["v1.1-small", "v1.1-base", "v1.1-large", "v1.1-xl", "v1.1-xxl"]


def size_config(size, **kw):
    """The T5Config of a ``--size`` name."""
    from cloudtik_amd.models.t5 import T5Config
    if size.startswith("v1.1-"):
        return T5Config.v1_1(size[len("v1.1-"):], **kw)
    return getattr(T5Config, _SIZES.get(size, size))(**kw)


def load_model(checkpoint, size, device, dtype):
    from cloudtik_amd.models.t5 import T5ForConditionalGeneration
    if checkpoint is None:
        torch.manual_seed(0)
        return T5ForConditionalGeneration(size_config(size, dropout_rate=0.0), device=device, dtype=dtype).eval()
    return T5ForConditionalGeneration.from_pretrained(checkpoint, device=device, dtype=dtype).eval()


def load_tokenizer(checkpoint):
    if checkpoint is None or not os.path.exists(os.path.join(checkpoint, "spiece.model")):
        return None
    try:
        from transformers import AutoTokenizer
        return AutoTokenizer.from_pretrained(checkpoint, local_files_only=True)
    except Exception as e:  # noqa: BLE001 - the example still runs on token ids
        print(f"no tokenizer ({e}); printing token ids")
        return None


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--checkpoint", default=None, help="local directory with config.json and the weights")
    ap.add_argument("--size", default="small", choices=["tiny", "small", "base", "large", "3b", "11b"] + _V1_1,
                    help="random-init topology")
    ap.add_argument("--text", action="append", help="source sentence (repeatable; needs the tokenizer)")
    ap.add_argument("--batch", type=int, default=2, help="random sources when there is no text")
    ap.add_argument("--source-len", type=int, default=24)
    ap.add_argument("--max-new-tokens", type=int, default=16)
    ap.add_argument("--num-beams", type=int, default=4)
    ap.add_argument("--length-penalty", type=float, default=1.0)
    ap.add_argument("--early-stopping", action="store_true")
    ap.add_argument("--do-sample", action="store_true", help="also draw samples (the flags below)")
    ap.add_argument("--temperature", type=float, default=1.0)
    ap.add_argument("--top-k", type=int, default=0, help="0: off")
    ap.add_argument("--top-p", type=float, default=1.0, help="1: off")
    ap.add_argument("--repetition-penalty", type=float, default=1.0)
    ap.add_argument("--num-return-sequences", type=int, default=1, help="samples per source")
    ap.add_argument("--seed", type=int, default=None, help="sampling seed (default: from torch's generator)")
    ap.add_argument("--no-repeat-ngram-size", type=int, default=0, help="no n-gram of this size twice (0: off)")
    ap.add_argument("--min-new-tokens", type=int, default=0, help="no EOS before this many new tokens")
    ap.add_argument("--min-length", type=int, default=0, help="the same, counting the start token as the library does")
    ap.add_argument("--bad-words", action="append", default=None, metavar="ID[,ID...]",
                    help="token ids of a sequence that must not appear (repeatable)")
    ap.add_argument("--task", default=None, help="use the checkpoint's task_specific_params of this task")
    ap.add_argument("--precision", default="bf16", choices=["bf16", "int8"],
                    help="int8: dynamic post-training quantization of every linear and the output head")
    a = ap.parse_args()

    gpu = torch.cuda.is_available()
    device = torch.device("cuda", 0) if gpu else torch.device("cpu")
    model = load_model(a.checkpoint, a.size, device, torch.bfloat16 if gpu else torch.float32)
    if a.precision == "int8":
        model = model.quantize_dynamic()
    tok = load_tokenizer(a.checkpoint)
    beam_kw = dict(max_new_tokens=a.max_new_tokens, num_beams=a.num_beams, length_penalty=a.length_penalty,
                   early_stopping=a.early_stopping)
    ban_kw = dict(no_repeat_ngram_size=a.no_repeat_ngram_size, min_new_tokens=a.min_new_tokens, min_length=a.min_length,
                  bad_words_ids=[[int(v) for v in w.split(",")] for w in a.bad_words] if a.bad_words else None)
    prefix = ""
    if a.task is not None:
        if a.checkpoint is None:
            ap.error("--task needs --checkpoint (the settings come from its config.json)")
        from cloudtik_amd.models.t5 import generate_kwargs_for_task
        task_kw, prefix = generate_kwargs_for_task(os.path.join(a.checkpoint, "config.json"), a.task)
        for name, value in task_kw.items():
            (ban_kw if name in ban_kw else beam_kw)[name] = value
        print(f"task {a.task}: {task_kw}, prefix {prefix!r}")
    if tok is not None and a.text:
        enc = tok([prefix + t for t in a.text], return_tensors="pt", padding=True)
        ids, mask = enc["input_ids"].to(device), enc["attention_mask"].to(device)
    else:
        g = torch.Generator().manual_seed(0)
        ids = torch.randint(2, model.cfg.vocab_size, (a.batch, a.source_len), generator=g).to(device)
        mask = torch.ones_like(ids)

    steps, beams = beam_kw["max_new_tokens"], beam_kw["num_beams"]
    greedy = model.generate(ids, mask, max_new_tokens=steps, **ban_kw)
    beam, score = model.generate(ids, mask, return_scores=True, **beam_kw, **ban_kw)
    show = (lambda row: tok.decode(row, skip_special_tokens=True)) if tok is not None else (lambda row: row.tolist())
    for i in range(ids.shape[0]):
        print(f"[{i}] greedy: {show(greedy[i])}")
        print(f"[{i}] beam {beams} (score {float(score[i]):.4f}): {show(beam[i])}")
    if a.do_sample:
        n = a.num_return_sequences
        samples = model.generate(ids, mask, max_new_tokens=steps, do_sample=True, temperature=a.temperature,
                                 top_k=a.top_k, top_p=a.top_p, repetition_penalty=a.repetition_penalty,
                                 num_return_sequences=n, seed=a.seed, **ban_kw)
        for i in range(ids.shape[0]):
            for j in range(n):                     # rows i * n .. i * n + n - 1 belong to source i
                print(f"[{i}] sample {j}: {show(samples[i * n + j])}")


if __name__ == "__main__":
    main()
