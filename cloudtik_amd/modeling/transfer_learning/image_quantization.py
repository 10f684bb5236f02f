"""Post-training static int8 quantization of the image classifier (reference modeling/
transfer_learning/image_classification/pytorch/image_classification_model.py:429-700:
``export_neural_compressor_config``, ``quantize``, ``benchmark_neural_compressor``, there backed by
Intel Neural Compressor on the CPU).

Module-level functions that take the ``ImageClassificationModel`` as their first argument; they
mirror ``quantization.TextQuantizationMixin`` and share its config format and helpers.  (The
hooks of the same names on the model class still raise NotImplementedError; switching them over
to these functions is a follow-up.)

The only approach is ``post_training_static_quant``: the convolutions of the quantized stages run
on ``ops.conv2d_i8_static`` with BatchNorm folded in and int8 activations between them
(``models.resnet_quant``), which needs one calibrated range per tensor -- there is no dynamic
(per-call) variant of an int8 convolution here.  ``quantize`` calibrates once on the first
``sampling_size`` examples and then walks ``resnet_quant.TRIALS`` -- all four stages; without
layer1; layer3 + layer4 -- until a trial's relative accuracy loss meets the criterion.
"""
from __future__ import annotations

import json
import os
import time
from typing import Dict

import torch

from .quantization import (APPROACH, STATIC_APPROACH, _batch_size, _calibration_batches, _sampling_size, build_config,
                           check_config_args, read_config, write_config)

_STATIC_ONLY = (f"image classification models support {STATIC_APPROACH!r} only: the int8 convolutions here are "
                f"static-only (calibrated ranges), there is no {APPROACH!r} for them")


def _check_dataset(dataset):
    from .datasets import ArrayImageDataset, ImageFolderDataset
    if not isinstance(dataset, (ImageFolderDataset, ArrayImageDataset)):
        raise NotImplementedError("image quantization has only been implemented for an ImageFolderDataset or an "
                                  "ArrayImageDataset")


def _describe(dataset) -> dict:
    return {"image_classification": {"num_examples": len(dataset), "image_size": int(dataset[0][0].shape[-1])}}


def export_quantization_config(model, config_file_path, dataset, batch_size, overwrite=False,
                               accuracy_criterion_relative=0.01, exit_policy_timeout=0, exit_policy_max_trials=50,
                               tuning_random_seed=9527, tuning_workspace='', approach=STATIC_APPROACH,
                               calibration_sampling_size=100):
    """Write the quantization / tuning config (YAML) for ``quantize`` and ``benchmark``.

    Raises FileExistsError when the file exists and ``overwrite`` is False, NotImplementedError for
    a dataset that is neither an ``ImageFolderDataset`` nor an ``ArrayImageDataset``, ValueError for
    a parameter outside its range -- ``approach='post_training_dynamic_quant'`` among them."""
    if os.path.isfile(config_file_path) and not overwrite:
        raise FileExistsError(f"A file already exists at: {config_file_path}. Provide a new file path or "
                              "set overwrite=True")
    _check_dataset(dataset)
    if approach == APPROACH:
        raise ValueError(_STATIC_ONLY)
    check_config_args(batch_size, accuracy_criterion_relative, exit_policy_timeout, exit_policy_max_trials,
                      tuning_random_seed, tuning_workspace, approach, calibration_sampling_size,
                      approaches=(STATIC_APPROACH,))
    if not tuning_workspace and os.getenv("OUTPUT_DIR", ""):
        tuning_workspace = os.path.join(os.environ["OUTPUT_DIR"], "nc_workspace")
    cfg = build_config(model.model_name, dataset, batch_size, accuracy_criterion_relative, exit_policy_timeout,
                       exit_policy_max_trials, tuning_random_seed, tuning_workspace, approach,
                       calibration_sampling_size, describe_dataset=_describe)
    write_config(cfg, config_file_path)


def _trial_accuracy(wrapper, dataset, batch_size: int) -> float:
    """Accuracy of ``wrapper`` (an ``ImageClassificationModel``) on ``dataset``."""
    return float(wrapper.evaluate(dataset, batch_size=batch_size)["accuracy"])


def _read_static(config_path: str) -> dict:
    cfg = read_config(config_path)
    if cfg["quantization"]["approach"] != STATIC_APPROACH:
        raise ValueError(_STATIC_ONLY)
    return cfg


def quantize(model, saved_model_dir, output_dir, config_path, dataset):
    """Quantize the model exported at ``saved_model_dir`` and write it to ``output_dir``.

    The float model is run once over the first ``sampling_size`` examples of ``dataset`` to
    calibrate the activation ranges; the float and the int8 accuracy are measured on ``dataset``,
    and while the relative loss exceeds the config's criterion the next trial of the ladder
    (``resnet_quant.TRIALS``) is taken, up to the exit policy's trial count / timeout.  Returns the
    written ``model.safetensors`` path, or None -- with nothing written -- when no trial met the
    criterion.

    Raises NotADirectoryError (``saved_model_dir``), FileNotFoundError (its model file, or the
    config), FileExistsError (``output_dir`` already holds a model), ValueError (no dataset, a
    config that is not static, an already quantized model), NotImplementedError (the dataset's
    type; a model that is not built from plain bottlenecks)."""
    from cloudtik_amd.models import resnet_quant
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
    cfg = _read_static(config_path)
    if dataset is None:
        raise ValueError(f"{STATIC_APPROACH} calibrates the activation ranges on a dataset; none was given")
    _check_dataset(dataset)
    tuning = cfg.get("tuning", {})
    criterion = float(tuning.get("accuracy_criterion", {}).get("relative", 0.01))
    policy = tuning.get("exit_policy", {})
    max_trials = int(policy.get("max_trials") or len(resnet_quant.TRIALS))
    timeout = float(policy.get("timeout") or 0)
    bs = _batch_size(cfg, "accuracy", 64)

    fp = type(model).load(saved_model_dir, device=model.device)
    if fp.quantization:
        raise ValueError(f"the model at {saved_model_dir} is already quantized")
    acc_fp = _trial_accuracy(fp, dataset, bs)
    n = min(_sampling_size(cfg), len(dataset))
    act_amax = resnet_quant.calibrate(fp.model, _calibration_batches(dataset, n, bs))   # once; the trials share it
    calibration = {"sampling_size": _sampling_size(cfg), "num_examples": n}
    t0, chosen, history = time.monotonic(), None, []
    for trial, sites in enumerate(resnet_quant.TRIALS[:max_trials], 1):
        if trial > 1 and timeout and time.monotonic() - t0 > timeout:
            break
        q = type(model).load(saved_model_dir, device=model.device)
        q.model = resnet_quant.QuantResNet.from_float(q.model, sites, act_amax)
        q.quantization = {"approach": STATIC_APPROACH}
        acc_q = _trial_accuracy(q, dataset, bs)
        loss = (acc_fp - acc_q) / acc_fp if acc_fp > 0 else 0.0
        history.append({"trial": trial, "sites": list(sites), "accuracy": acc_q, "relative_loss": loss})
        if loss <= criterion:
            chosen = (trial, q, acc_q)
            break
    if chosen is None:
        return None
    trial, q, acc_q = chosen
    q.quantization = {"approach": STATIC_APPROACH, "sites": list(q.model.sites), "act_amax": act_amax,
                      "calibration": calibration, "accuracy": {"fp32": acc_fp, "int8": acc_q},
                      "accuracy_criterion_relative": criterion, "trial": trial, "trials": history}
    os.makedirs(output_dir, exist_ok=True)
    return q.export(output_dir)


def benchmark(model, saved_model_dir, config_path=None, mode='performance', model_type='fp32', dataset=None,
              batch_size=None, image_size=224, warmup=5, iters=20) -> Dict[str, float]:
    """Measure the model exported (``model_type='fp32'``: the unquantized export in its own dtype)
    or quantized (``'int8'``) at ``saved_model_dir``.  ``mode='performance'``: forward latency of
    one ``batch_size`` x 3 x ``image_size``^2 batch (HIP events on the GPU, ``perf_counter`` on the
    CPU; ``warmup`` calls excluded); ``mode='accuracy'``: accuracy on ``dataset``.  Returns the
    result dict and prints it as one JSON line."""
    if mode not in ('performance', 'accuracy'):
        raise ValueError(f"Invalid mode: {mode}. Expected 'performance' or 'accuracy'.")
    if model_type not in ('fp32', 'int8'):
        raise ValueError(f"Invalid model_type: {model_type}. Expected 'fp32' or 'int8'.")
    if not os.path.isdir(saved_model_dir):
        raise NotADirectoryError(f"The saved model directory ({saved_model_dir}) does not exist.")
    if config_path is not None and not os.path.isfile(config_path):
        raise FileNotFoundError(f"The config file was not found at: {config_path}")
    cfg = _read_static(config_path) if config_path is not None else {}
    m = type(model).load(saved_model_dir, device=model.device)
    if (model_type == 'int8') != bool(m.quantization):
        raise ValueError(f"model_type={model_type!r} but the model at {saved_model_dir} is "
                         f"{'quantized' if m.quantization else 'not quantized'}")
    if mode == 'accuracy':
        if dataset is None:
            raise ValueError("accuracy mode needs a dataset")
        res = {"accuracy": _trial_accuracy(m, dataset, batch_size or _batch_size(cfg, "accuracy", 64))}
    else:
        bs = int(batch_size or _batch_size(cfg, "performance", 32))
        res = time_forward(m, bs, int(image_size), int(warmup), int(iters))
    print(json.dumps(dict(res, mode=mode, model_type=model_type, model_name=m.model_name)), flush=True)
    return res


@torch.no_grad()
def time_forward(m, batch_size: int, image_size: int, warmup: int, iters: int) -> Dict[str, float]:
    dev = m.device
    x = torch.randn(batch_size, 3, image_size, image_size, generator=torch.Generator().manual_seed(0))
    x = x.to(dev, m.dtype)
    if dev.type == "cuda":
        x = x.contiguous(memory_format=torch.channels_last)
    m.model.eval()
    for _ in range(warmup):
        m.model(x)
    if dev.type == "cuda":
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(dev)
        start.record()
        for _ in range(iters):
            m.model(x)
        end.record()
        torch.cuda.synchronize(dev)
        ms = start.elapsed_time(end) / iters
    else:
        t0 = time.perf_counter()
        for _ in range(iters):
            m.model(x)
        ms = (time.perf_counter() - t0) * 1e3 / iters
    return {"latency_ms": ms, "throughput": batch_size * 1e3 / ms, "batch_size": batch_size,
            "image_size": image_size, "warmup": warmup, "iters": iters}
