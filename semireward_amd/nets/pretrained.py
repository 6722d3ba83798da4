"""Pretrained backbone weights from checkpoints already on disk: where the reference finds them offline, and the rules it loads them by.

Nothing is downloaded.  Two lookups, the places the reference's own loaders read when they are offline:

  * ViT / WRN, ``load_checkpoint(model, path)`` (semilearn/nets/utils.py): ``path`` itself when it is a file, else the file
    ``torch.hub.load_state_dict_from_url`` would have cached for the URL, ``<torch.hub.get_dir()>/checkpoints/<basename of the URL path>``.
  * BERT / Wav2Vec2 / HuBERT, ``from_pretrained(<model name>)``: a ``pretrained_path`` directory (an engine extension: the reference ignores the
    key for these nets), else the Hugging Face hub-cache snapshot ``<hub cache>/models--<org>--<name>/snapshots/<refs/main>/`` with
    ``config.json`` and ``model.safetensors`` or ``pytorch_model.bin``.

When nothing is found the builder keeps its random init and one warning line names every path tried.  Loading has ``strict=False``
semantics with torch's shape check: keys the file lacks keep their init, keys the model lacks are reported and ignored, a shape mismatch
raises.  The tensors go into the flat parameter block through ``ModuleSurface.load_state_dict``, which refreshes the operand copies.
"""
import json
import math
import os
import struct
import sys
import urllib.parse

import torch
import torch.nn.functional as F


def _warn(msg):
    print("warning: " + msg, file=sys.stderr, flush=True)


# ---- loading into an engine backbone -----------------------------------------------------------------------------------------------------
def load_weights(model, sd):
    """``nn.Module.load_state_dict(sd, strict=False)`` on the flat block: returns (missing, unexpected) key lists.  Parameters and buffers
    (BatchNorm running statistics, ``num_batches_tracked``) are checked for shape first, so a mismatch raises before anything is written."""
    shapes = {n: tuple(s) for n, s in model.names_shapes}
    shapes.update({k: tuple(v.shape) for k, v in model.buffers.items()})
    take, unexpected = {}, []
    for k, v in sd.items():
        if k not in shapes:
            unexpected.append(k)
            continue
        if tuple(v.shape) != shapes[k]:
            raise RuntimeError("size mismatch for %s: copying a param with shape %s from checkpoint, the shape in current model is %s."
                               % (k, torch.Size(v.shape), torch.Size(shapes[k])))
        take[k] = v
    missing = [k for k in shapes if k not in take]
    model.load_state_dict(take, strict=False)
    return missing, unexpected


def _report(model, source, missing, unexpected):
    print("%s: loaded %s (missing_keys=%s, unexpected_keys=%s)" % (type(model).__name__, source, missing, unexpected), file=sys.stderr, flush=True)


# ---- ViT / WRN: load_checkpoint ----------------------------------------------------------------------------------------------------------
def torch_hub_file(path):
    """(checkpoint file or None, paths tried) for a ``pretrain_path``: the path itself, else the torch-hub cache entry of the URL."""
    if not path:
        return None, []
    if os.path.isfile(path):
        return path, [path]
    tried = [path]
    name = os.path.basename(urllib.parse.urlparse(path).path)
    if name:
        cached = os.path.join(torch.hub.get_dir(), "checkpoints", name)
        tried.append(cached)
        if os.path.isfile(cached):
            return cached, tried
    return None, tried


def resize_pos_embed(posemb, new_shape, num_tokens=1):
    """Position embeddings [1, tokens + grid^2, D] resampled to the grid of ``new_shape``: the class token is kept, the grid goes through a
    bicubic resample (align_corners False) on the CPU in fp32, as the reference's loader does it."""
    posemb = posemb.detach().to("cpu", torch.float32)
    tok, grid = posemb[:, :num_tokens], posemb[0, num_tokens:]
    gs_old, gs_new = int(math.sqrt(grid.shape[0])), int(math.sqrt(new_shape[1] - num_tokens))
    grid = grid.reshape(1, gs_old, gs_old, -1).permute(0, 3, 1, 2)
    grid = F.interpolate(grid, size=[gs_new, gs_new], mode="bicubic", align_corners=False)
    grid = grid.permute(0, 2, 3, 1).reshape(1, gs_new * gs_new, -1)
    return torch.cat([tok, grid], dim=1)


def checkpoint_state_dict(checkpoint, model):
    """The reference's key rules for a ViT / WRN checkpoint: ``checkpoint['model']``, a leading ``module`` component stripped, classifier
    heads (keys starting with fc / classifier / mlp / head) dropped, ``pos_embed`` resampled to the model's grid."""
    out = {}
    for k, v in checkpoint["model"].items():
        if k.startswith("module"):
            k = ".".join(k.split(".")[1:])
        if k.startswith(("fc", "classifier", "mlp", "head")):
            continue
        if k == "pos_embed" and k in model.offsets:
            v = resize_pos_embed(v, model.offsets[k][1])
        out[k] = v
    return out


def load_checkpoint(model, checkpoint_path):
    """``semilearn.nets.utils.load_checkpoint`` on an engine backbone, without the download: returns the model, with its random init when
    no file is found."""
    path, tried = torch_hub_file(checkpoint_path)
    if path is None:
        _warn("%s: pretrained checkpoint not found (tried %s); keeping the random init" % (type(model).__name__, ", ".join(tried) or "no path"))
        return model
    checkpoint = torch.load(path, map_location="cpu", weights_only=True)
    missing, unexpected = load_weights(model, checkpoint_state_dict(checkpoint, model))
    _report(model, path, missing, unexpected)
    return model


# ---- BERT / Wav2Vec2 / HuBERT: from_pretrained ---------------------------------------------------------------------------------------------
WEIGHT_FILES = ("model.safetensors", "pytorch_model.bin")


def hf_hub_cache():
    if os.environ.get("HF_HUB_CACHE"):
        return os.environ["HF_HUB_CACHE"]
    if os.environ.get("HF_HOME"):
        return os.path.join(os.environ["HF_HOME"], "hub")
    return os.path.join(os.path.expanduser("~"), ".cache", "huggingface", "hub")


def _complete(d):
    return os.path.isfile(os.path.join(d, "config.json")) and any(os.path.isfile(os.path.join(d, f)) for f in WEIGHT_FILES)


def find_snapshot(name, pretrained_path=None):
    """(directory or None, paths tried): ``pretrained_path`` when it is a directory with ``config.json`` and weights, else the hub-cache
    snapshot that ``refs/main`` of model ``name`` points at."""
    tried = []
    if pretrained_path:
        tried.append(pretrained_path)
        if os.path.isdir(pretrained_path) and _complete(pretrained_path):
            return pretrained_path, tried
    if name:
        repo = os.path.join(hf_hub_cache(), "models--" + name.replace("/", "--"))
        ref = os.path.join(repo, "refs", "main")
        if os.path.isfile(ref):
            with open(ref) as f:
                snap = os.path.join(repo, "snapshots", f.read().strip())
            tried.append(snap)
            if _complete(snap):
                return snap, tried
        else:
            tried.append(ref)
    return None, tried


_ST_DTYPES = {"F64": torch.float64, "F32": torch.float32, "F16": torch.float16, "BF16": torch.bfloat16, "I64": torch.int64,
              "I32": torch.int32, "I16": torch.int16, "I8": torch.int8, "U8": torch.uint8, "BOOL": torch.bool}


def read_safetensors(path):
    """A ``.safetensors`` file (8-byte little-endian header length, JSON header, raw little-endian data) -> dict of CPU tensors."""
    with open(path, "rb") as f:
        n = struct.unpack("<Q", f.read(8))[0]
        header = json.loads(f.read(n))
        data = bytearray(f.read())
    out = {}
    for k, v in header.items():
        if k == "__metadata__":
            continue
        a, b = v["data_offsets"]
        dt = _ST_DTYPES[v["dtype"]]
        raw = torch.frombuffer(data, dtype=torch.uint8, count=b - a, offset=a).clone() if b > a else torch.empty(0, dtype=torch.uint8)
        out[k] = raw.view(dt).reshape(v["shape"])
    return out


def read_snapshot(d):
    """(config.json dict, state dict) of a snapshot directory: ``model.safetensors``, else ``pytorch_model.bin``."""
    with open(os.path.join(d, "config.json")) as f:
        config = json.load(f)
    st, pt = os.path.join(d, WEIGHT_FILES[0]), os.path.join(d, WEIGHT_FILES[1])
    sd = read_safetensors(st) if os.path.isfile(st) else torch.load(pt, map_location="cpu", weights_only=True)
    return config, sd


# family -> (task-model prefix of the checkpoint, the engine's prefix)
_PREFIX = {"bert": ("bert.", "bert."), "wav2vec2": ("wav2vec2.", "model."), "hubert": ("hubert.", "model.")}
_HEADS = ("cls.", "lm_head.", "quantizer.", "project_")
_RENAME = {"gamma": "weight", "beta": "bias", "weight_g": "parametrizations.weight.original0", "weight_v": "parametrizations.weight.original1"}


def hf_state_dict(sd, family):
    """A transformers checkpoint in the engine's names: task heads and ``position_ids`` dropped, the task-model prefix stripped, legacy
    ``gamma`` / ``beta`` and weight-norm ``weight_g`` / ``weight_v`` names renamed, the engine's prefix added."""
    strip, add = _PREFIX[family]
    out = {}
    for k, v in sd.items():
        if k.startswith(_HEADS) or k.endswith("position_ids"):
            continue
        if k.startswith(strip):
            k = k[len(strip):]
        head, _, last = k.rpartition(".")
        if last in _RENAME:
            k = head + "." + _RENAME[last]
        out[add + k] = v
    return out


# config.json field -> (engine config attribute, or None and the one value the engine supports)
_BERT_GEOMETRY = (("hidden_size", "hidden", None), ("num_hidden_layers", "layers", None), ("num_attention_heads", "heads", None),
                  ("intermediate_size", "inter", None), ("vocab_size", "vocab", None), ("max_position_embeddings", "max_pos", None),
                  ("type_vocab_size", None, 2), ("layer_norm_eps", "eps", None), ("hidden_act", None, "gelu"))
_AUDIO_GEOMETRY = (("hidden_size", "hidden", None), ("num_hidden_layers", "layers", None), ("num_attention_heads", "heads", None),
                   ("intermediate_size", "inter", None), ("layer_norm_eps", "eps", None), ("hidden_act", None, "gelu"),
                   ("conv_dim", "conv_dim", None), ("conv_kernel", "conv_kernel", None), ("conv_stride", "conv_stride", None),
                   ("conv_bias", None, False), ("feat_extract_norm", None, "group"), ("do_stable_layer_norm", None, False),
                   ("num_conv_pos_embeddings", "pos_k", None), ("num_conv_pos_embedding_groups", "pos_groups", None))
# config.json train-mode settings -> W2vConfig attribute
_AUDIO_TRAIN = (("hidden_dropout", "p_hidden"), ("attention_dropout", "p_attn"), ("activation_dropout", "p_act"), ("feat_proj_dropout", "p_featproj"),
                ("layerdrop", "layerdrop"), ("mask_time_prob", "mask_time_prob"), ("mask_time_length", "mask_time_length"),
                ("mask_time_min_masks", "mask_time_min_masks"))


def _norm(v):
    return tuple(v) if isinstance(v, (list, tuple)) else v


def _check_geometry(config, cfg, fields, source):
    for key, attr, want in fields:
        want = getattr(cfg, attr) if attr is not None else want
        if key not in config:
            raise NotImplementedError("%s/config.json: no %r field; the engine needs %r" % (source, key, want))
        if _norm(config[key]) != _norm(want):
            raise NotImplementedError("%s/config.json: %s = %r, the engine's builder has %r" % (source, key, config[key], want))


def apply_bert_config(config, cfg, source):
    """Checks ``config.json`` against the BertConfig of the builder and takes its dropout probability (``from_pretrained`` trains with the
    checkpoint's config).  The engine has one encoder dropout probability, so the two of the file must agree."""
    _check_geometry(config, cfg, _BERT_GEOMETRY, source)
    ph, pa = config.get("hidden_dropout_prob", cfg.p_drop), config.get("attention_probs_dropout_prob", cfg.p_drop)
    if ph != pa:
        raise NotImplementedError("%s/config.json: hidden_dropout_prob %r != attention_probs_dropout_prob %r; the engine has one encoder "
                                  "dropout probability" % (source, ph, pa))
    cfg.p_drop = ph
    cfg.p_head = 0.1                 # the classification head's own Dropout(p=0.1) (bert.py:14), whatever the encoder's is


def apply_audio_config(config, cfg, source):
    """Checks ``config.json`` against the W2vConfig of the builder and takes its dropout, LayerDrop and SpecAugment settings."""
    _check_geometry(config, cfg, _AUDIO_GEOMETRY, source)
    if config.get("mask_feature_prob", 0.0) > 0:
        raise NotImplementedError("%s/config.json: mask_feature_prob = %r; the engine has no feature-axis SpecAugment" % (source, config["mask_feature_prob"]))
    for key, attr in _AUDIO_TRAIN:
        if key in config:
            setattr(cfg, attr, config[key])
    if not config.get("apply_spec_augment", True):
        cfg.mask_time_prob = 0.0     # transformers masks only when apply_spec_augment and mask_time_prob > 0


def find_hf_weights(model_name, name, pretrained_path):
    """(config dict, state dict, source) of the snapshot a BERT / Wav2Vec2 / HuBERT builder starts from, or None with a warning."""
    d, tried = find_snapshot(name, pretrained_path)
    if d is None:
        if tried:
            _warn("%s: pretrained weights of %s not found (tried %s); keeping the random init" % (model_name, name or pretrained_path, ", ".join(tried)))
        return None
    config, sd = read_snapshot(d)
    return config, sd, d


def load_hf(model, sd, family, source):
    """Loads a transformers checkpoint (``hf_state_dict``) into the engine model; the classifier keeps its init, as in the reference."""
    missing, unexpected = load_weights(model, hf_state_dict(sd, family))
    _report(model, source, missing, unexpected)
    return missing, unexpected
