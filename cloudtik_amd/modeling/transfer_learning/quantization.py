"""Post-training int8 quantization of the text classifier (reference modeling/
transfer_learning/model.py:107-190 and text_classification/pytorch/hugging_face/
text_classification_model.py:575-780: ``export_neural_compressor_config``, ``quantize``,
``benchmark_neural_compressor``, there backed by Intel Neural Compressor on the CPU).

Here the approach ``post_training_dynamic_quant`` -- int8 weights, activations quantized per
call -- runs through the in-tree HIP kernels (``ops.quant``, ``models.bert_quant``).  The tuning
loop is a short ladder of site sets instead of INC's search: a trial is accepted when its
relative accuracy loss on the evaluation dataset is within the configured criterion.

``post_training_static_quant`` keeps the int8 weights and replaces the per-token activation
scales by one range per site and layer, calibrated on the first ``sampling_size`` examples of the
dataset (``models.bert_quant.calibrate``).  The ranges are written into the quantization block of
``model_config.json``; with them the int8 activations come straight out of the LayerNorm and GEMM
epilogues instead of separate quantize passes.
"""
from __future__ import annotations

import json
import os
import time
from typing import Dict, List, Optional

import torch

APPROACH = "post_training_dynamic_quant"
STATIC_APPROACH = "post_training_static_quant"
APPROACHES = (APPROACH, STATIC_APPROACH)

# the trial ladder: all four linears; then without ffn2 (the largest K, fed by the post-GELU
# tensor); then the two linears whose inputs are LayerNorm outputs
TRIALS = (("qkv", "out", "ffn1", "ffn2"), ("qkv", "out", "ffn1"), ("qkv", "ffn1"))


def _bad_int(v, lowest):
    return (v and not isinstance(v, int)) or v is None or v < lowest


def build_config(model_name: str, dataset, batch_size: int, accuracy_criterion_relative, exit_policy_timeout,
                 exit_policy_max_trials, tuning_random_seed, tuning_workspace, approach=APPROACH,
                 calibration_sampling_size=100, describe_dataset=None) -> dict:
    """``describe_dataset(dataset)`` gives the ``dataset`` entry of the two dataloader blocks; the
    default describes a ``TextClassificationDataset``."""
    if describe_dataset is None:
        describe_dataset = lambda d: {"text_classification": {"num_examples": len(d),
                                                              "max_length": int(d.ids.shape[1])}}
    loader = lambda: {"batch_size": batch_size, "dataset": describe_dataset(dataset)}
    tuning = {"accuracy_criterion": {"relative": accuracy_criterion_relative},
              "exit_policy": {"timeout": exit_policy_timeout, "max_trials": exit_policy_max_trials},
              "random_seed": tuning_random_seed}
    if tuning_workspace:
        tuning["workspace"] = {"path": tuning_workspace}
    quantization = {"approach": approach}
    if approach == STATIC_APPROACH:
        quantization["calibration"] = {"sampling_size": calibration_sampling_size}
    return {"version": 1.0,
            "model": {"name": model_name, "framework": "cloudtik_amd"},
            "quantization": quantization,
            "evaluation": {"accuracy": {"metric": {"topk": 1}, "dataloader": loader()},
                           "performance": {"configs": {"num_of_instance": 1}, "dataloader": loader()}},
            "tuning": tuning}


def read_config(path: str) -> dict:
    import yaml
    with open(path) as f:
        cfg = yaml.safe_load(f) or {}
    approach = cfg.get("quantization", {}).get("approach")
    if approach not in APPROACHES:
        raise ValueError(f"unsupported quantization approach {approach!r}; this library implements "
                         f"{' and '.join(map(repr, APPROACHES))}")
    return cfg


def _sampling_size(cfg: dict) -> int:
    n = cfg.get("quantization", {}).get("calibration", {}).get("sampling_size", 100)
    if _bad_int(n, 1) or isinstance(n, bool):
        raise ValueError(f"Invalid calibration sampling size ({n}) in the config. Expected a positive integer.")
    return n


def _batch_size(cfg: dict, section: str, default: int) -> int:
    return int(cfg.get("evaluation", {}).get(section, {}).get("dataloader", {}).get("batch_size") or default)


def check_config_args(batch_size, accuracy_criterion_relative, exit_policy_timeout, exit_policy_max_trials,
                      tuning_random_seed, tuning_workspace, approach, calibration_sampling_size,
                      approaches=APPROACHES):
    """The value checks of ``export_quantization_config`` (ValueError), shared by the text mixin
    and the image workflow."""
    if _bad_int(batch_size, 1) or isinstance(batch_size, bool):
        raise ValueError(f"Invalid value for batch size ({batch_size}). Expected a positive integer.")
    if (accuracy_criterion_relative and not isinstance(accuracy_criterion_relative, float)) or \
            accuracy_criterion_relative is None or not (0.0 <= accuracy_criterion_relative <= 1.0):
        raise ValueError(f"Invalid value for the accuracy criterion ({accuracy_criterion_relative}). "
                         "Expected a float value between 0.0 and 1.0")
    if _bad_int(exit_policy_timeout, 0):
        raise ValueError(f"Invalid value for the exit policy timeout ({exit_policy_timeout}). "
                         "Expected a positive integer or 0.")
    if _bad_int(exit_policy_max_trials, 1):
        raise ValueError(f"Invalid value for max trials ({exit_policy_max_trials}). "
                         "Expected an integer greater than 0.")
    if _bad_int(tuning_random_seed, 0):
        raise ValueError(f"Invalid value for tuning random seed ({tuning_random_seed}). "
                         "Expected a positive integer.")
    if not isinstance(tuning_workspace, str):
        raise ValueError("Invalid value for the tuning workspace directory. Expected a string.")
    if approach not in approaches:
        raise ValueError(f"Invalid value for the approach ({approach!r}). Expected one of {list(approaches)}.")
    if _bad_int(calibration_sampling_size, 1) or isinstance(calibration_sampling_size, bool):
        raise ValueError(f"Invalid value for the calibration sampling size ({calibration_sampling_size}). "
                         "Expected a positive integer.")


def write_config(cfg: dict, config_file_path: str):
    import yaml
    parent = os.path.dirname(config_file_path)
    if parent:
        os.makedirs(parent, exist_ok=True)
    with open(config_file_path, "w") as f:
        yaml.safe_dump(cfg, f, sort_keys=False)


class TextQuantizationMixin:
    """``export_quantization_config`` / ``quantize`` / ``benchmark`` of ``TextClassificationModel``
    and the reference-named aliases."""

    quantization: Optional[dict] = None          # the "quantization" block of a loaded int8 model

    # ------------------------------------------------------------------ config
    def export_quantization_config(self, config_file_path, dataset, batch_size, overwrite=False,
                                   accuracy_criterion_relative=0.01, exit_policy_timeout=0,
                                   exit_policy_max_trials=50, tuning_random_seed=9527, tuning_workspace='',
                                   approach=APPROACH, calibration_sampling_size=100):
        """Write the quantization / tuning config (YAML) for ``quantize`` and ``benchmark``.
        ``approach`` is ``post_training_dynamic_quant`` or ``post_training_static_quant``; the
        static one calibrates on the first ``calibration_sampling_size`` examples.

        Raises FileExistsError when the file exists and ``overwrite`` is False, NotImplementedError
        for a dataset that is not a ``TextClassificationDataset``, ValueError for a parameter
        outside its range."""
        from .datasets import TextClassificationDataset
        if os.path.isfile(config_file_path) and not overwrite:
            raise FileExistsError(f"A file already exists at: {config_file_path}. Provide a new file path or "
                                  "set overwrite=True")
        if not isinstance(dataset, TextClassificationDataset):
            raise NotImplementedError("quantization has only been implemented for text classification models "
                                      "with a TextClassificationDataset")
        check_config_args(batch_size, accuracy_criterion_relative, exit_policy_timeout, exit_policy_max_trials,
                          tuning_random_seed, tuning_workspace, approach, calibration_sampling_size)
        if not tuning_workspace and os.getenv("OUTPUT_DIR", ""):
            tuning_workspace = os.path.join(os.environ["OUTPUT_DIR"], "nc_workspace")
        cfg = build_config(self.model_name, dataset, batch_size, accuracy_criterion_relative, exit_policy_timeout,
                           exit_policy_max_trials, tuning_random_seed, tuning_workspace, approach,
                           calibration_sampling_size)
        write_config(cfg, config_file_path)

    def export_neural_compressor_config(self, config_file_path, dataset, batch_size, overwrite=False,
                                        resize_interpolation='bicubic', accuracy_criterion_relative=0.01,
                                        exit_policy_timeout=0, exit_policy_max_trials=50, tuning_random_seed=9527,
                                        tuning_workspace='', approach=APPROACH, calibration_sampling_size=100):
        """The reference's name and signature (``resize_interpolation`` is validated and unused,
        as for the reference's text models), then ``approach`` and ``calibration_sampling_size``."""
        if resize_interpolation not in ('bilinear', 'nearest', 'bicubic'):
            raise ValueError(f"Invalid value for resize interpolation ({resize_interpolation}). Expected one of "
                             "the following values: bilinear, nearest, bicubic")
        return self.export_quantization_config(config_file_path, dataset, batch_size, overwrite,
                                               accuracy_criterion_relative, exit_policy_timeout,
                                               exit_policy_max_trials, tuning_random_seed, tuning_workspace,
                                               approach, calibration_sampling_size)

    # ------------------------------------------------------------------ quantize
    def _trial_accuracy(self, wrapper, dataset, batch_size: int) -> float:
        """Accuracy of ``wrapper`` (a model object of this class) on ``dataset``."""
        return float(wrapper.evaluate(dataset, batch_size=batch_size)["accuracy"])

    def quantize(self, saved_model_dir, output_dir, config_path, dataset=None):
        """Quantize the model exported at ``saved_model_dir`` and write it to ``output_dir``.

        With a ``dataset`` the float and the int8 accuracy are measured; while the relative loss
        exceeds the config's criterion the next trial of the ladder (``TRIALS``) is taken, up to
        the exit policy's trial count / timeout.  Returns the written ``model.safetensors`` path,
        or None -- with nothing written -- when no trial met the criterion.

        A ``post_training_static_quant`` config needs the ``dataset``: the float model is run once
        over its first ``sampling_size`` examples to calibrate the activation ranges, which every
        trial then shares.

        Raises NotADirectoryError (``saved_model_dir``), FileNotFoundError (its model file, or the
        config), FileExistsError (``output_dir`` already holds a model), ValueError (a static
        config without a dataset)."""
        from cloudtik_amd.models import bert_quant
        if not os.path.isdir(saved_model_dir):
            raise NotADirectoryError(f"The saved model directory ({saved_model_dir}) does not exist.")
        if not os.path.isfile(os.path.join(saved_model_dir, "model.safetensors")):
            raise FileNotFoundError(f"The saved model directory ({saved_model_dir}) should have a "
                                    "model.safetensors file")
        if not os.path.isfile(config_path):
            raise FileNotFoundError(f"The config file was not found at: {config_path}")
        out_model = os.path.join(output_dir, "model.safetensors")
        if os.path.exists(out_model):
            raise FileExistsError(f"A saved model already exists at: {out_model}")
        cfg = read_config(config_path)
        approach = cfg["quantization"]["approach"]
        static = approach == STATIC_APPROACH
        if static and dataset is None:
            raise ValueError(f"{STATIC_APPROACH} calibrates the activation ranges on a dataset; none was given")
        tuning = cfg.get("tuning", {})
        criterion = float(tuning.get("accuracy_criterion", {}).get("relative", 0.01))
        policy = tuning.get("exit_policy", {})
        max_trials = int(policy.get("max_trials") or len(TRIALS))
        timeout = float(policy.get("timeout") or 0)
        bs = _batch_size(cfg, "accuracy", 64)

        fp = type(self).load(saved_model_dir, device=self.device)
        if fp.quantization:
            raise ValueError(f"the model at {saved_model_dir} is already quantized")
        acc_fp = self._trial_accuracy(fp, dataset, bs) if dataset is not None else None
        act_amax, calibration = None, None
        if static:                                        # once, on the float model; the trials share it
            n = min(_sampling_size(cfg), len(dataset))
            act_amax = bert_quant.calibrate(fp.model, _calibration_batches(dataset, n, bs))
            calibration = {"sampling_size": _sampling_size(cfg), "num_examples": n}
        t0, chosen, history = time.monotonic(), None, []
        for trial, sites in enumerate(TRIALS[:max_trials], 1):
            if trial > 1 and timeout and time.monotonic() - t0 > timeout:
                break
            q = type(self).load(saved_model_dir, device=self.device)
            q.model = bert_quant.QuantBertClassifier.from_float(q.model, sites, act_amax=act_amax)
            q.quantization = {"approach": approach}
            acc_q = self._trial_accuracy(q, dataset, bs) if dataset is not None else None
            loss = None
            if acc_q is not None:
                loss = (acc_fp - acc_q) / acc_fp if acc_fp > 0 else 0.0
            history.append({"trial": trial, "sites": list(sites), "accuracy": acc_q, "relative_loss": loss})
            if loss is None or loss <= criterion:
                chosen = (trial, q, acc_q)
                break
        if chosen is None:
            return None
        trial, q, acc_q = chosen
        q.quantization = {"approach": approach, "sites": q.model.sites_per_layer}
        if static:
            q.quantization.update(act_amax=act_amax, calibration=calibration)
        q.quantization.update({"accuracy": {"fp32": acc_fp, "int8": acc_q},
                               "accuracy_criterion_relative": criterion, "trial": trial, "trials": history})
        os.makedirs(output_dir, exist_ok=True)
        return q.export(output_dir)

    # ------------------------------------------------------------------ benchmark
    def benchmark(self, saved_model_dir, config_path=None, mode='performance', model_type='fp32', dataset=None,
                  batch_size=None, seq_len=128, warmup=5, iters=20) -> Dict[str, float]:
        """Measure the model exported (``model_type='fp32'``: the unquantized export in its own
        dtype) or quantized (``'int8'``) at ``saved_model_dir``.  ``mode='performance'``: forward
        latency of one ``batch_size`` x ``seq_len`` batch (HIP events on the GPU, ``perf_counter``
        on the CPU; ``warmup`` calls excluded); ``mode='accuracy'``: accuracy on ``dataset``.
        Returns the result dict and prints it as one JSON line."""
        if mode not in ('performance', 'accuracy'):
            raise ValueError(f"Invalid mode: {mode}. Expected 'performance' or 'accuracy'.")
        if model_type not in ('fp32', 'int8'):
            raise ValueError(f"Invalid model_type: {model_type}. Expected 'fp32' or 'int8'.")
        if not os.path.isdir(saved_model_dir):
            raise NotADirectoryError(f"The saved model directory ({saved_model_dir}) does not exist.")
        if config_path is not None and not os.path.isfile(config_path):
            raise FileNotFoundError(f"The config file was not found at: {config_path}")
        cfg = read_config(config_path) if config_path is not None else {}
        m = type(self).load(saved_model_dir, device=self.device)
        if (model_type == 'int8') != bool(m.quantization):
            raise ValueError(f"model_type={model_type!r} but the model at {saved_model_dir} is "
                             f"{'quantized' if m.quantization else 'not quantized'}")
        if mode == 'accuracy':
            if dataset is None:
                raise ValueError("accuracy mode needs a dataset")
            res = {"accuracy": self._trial_accuracy(m, dataset, batch_size or _batch_size(cfg, "accuracy", 64))}
        else:
            bs = int(batch_size or _batch_size(cfg, "performance", 32))
            res = _time_forward(m, bs, int(seq_len), int(warmup), int(iters))
        print(json.dumps(dict(res, mode=mode, model_type=model_type, model_name=m.model_name)), flush=True)
        return res

    def benchmark_neural_compressor(self, saved_model_dir, inc_config_path, mode='performance', model_type='fp32'):
        """The reference's name and signature."""
        return self.benchmark(saved_model_dir, inc_config_path, mode=mode, model_type=model_type)


def _calibration_batches(dataset, n: int, batch_size: int):
    """The first ``n`` examples of ``dataset`` in order, ``batch_size`` at a time."""
    from torch.utils.data import DataLoader, Subset
    return DataLoader(Subset(dataset, range(n)), batch_size=batch_size)


@torch.no_grad()
def _time_forward(m, batch_size: int, seq_len: int, warmup: int, iters: int) -> Dict[str, float]:
    dev = m.device
    g = torch.Generator().manual_seed(0)
    seq_len = min(seq_len, m.cfg.max_position_embeddings)
    ids = torch.randint(1000 if m.cfg.vocab_size > 2000 else 1, m.cfg.vocab_size, (batch_size, seq_len),
                        generator=g).to(dev)
    mask = torch.ones(batch_size, seq_len, dtype=torch.long, device=dev)
    m.model.eval()
    for _ in range(warmup):
        m.model(ids, mask)
    if dev.type == "cuda":
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(dev)
        start.record()
        for _ in range(iters):
            m.model(ids, mask)
        end.record()
        torch.cuda.synchronize(dev)
        ms = start.elapsed_time(end) / iters
    else:
        t0 = time.perf_counter()
        for _ in range(iters):
            m.model(ids, mask)
        ms = (time.perf_counter() - t0) * 1e3 / iters
    m.model.train(not m.quantization)
    return {"latency_ms": ms, "throughput": batch_size * 1e3 / ms, "batch_size": batch_size, "seq_len": seq_len,
            "warmup": warmup, "iters": iters}
