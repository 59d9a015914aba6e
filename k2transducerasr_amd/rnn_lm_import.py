"""Import a neural LM: a torch state dict of icefall's ``RnnLmModel`` -> ``.k2w``.

icefall saves ``{"model": state_dict, ...}``; a bare state dict is taken as well.  The tensors keep their names and torch layout
(``input_embedding.weight``, ``rnn.weight_ih_l{k}``, ``rnn.weight_hh_l{k}``, ``rnn.bias_ih_l{k}``, ``rnn.bias_hh_l{k}``,
``output_linear.weight``, ``output_linear.bias``); the dimensions are read off their shapes.  With ``tie_weights`` the output matrix
must be the embedding and is left out of the file.

    python -m k2transducerasr_amd.rnn_lm_import epoch-30.pt rnn_lm.k2w [--sos-id 1] [--eos-id 1] [--tie-weights]
"""
from __future__ import annotations

import argparse
import re
from typing import Mapping

import numpy as np

from .synth import write_rnn_lm


def _np(t) -> np.ndarray:
    if hasattr(t, "detach"):
        t = t.detach().cpu().float().numpy()
    return np.ascontiguousarray(t, dtype=np.float32)


def import_state_dict(state_dict: Mapping, path: str, sos_id: int = 1, eos_id: int = 1, tie_weights: bool = False) -> dict:
    """write `path` from a state dict (icefall's {"model": ...} or a bare one); returns the metadata's dimensions"""
    sd = state_dict["model"] if "model" in state_dict and isinstance(state_dict["model"], Mapping) else state_dict
    sd = {k[7:] if k.startswith("module.") else k: v for k, v in sd.items()}
    layers = sorted(int(m.group(1)) for k in sd for m in [re.fullmatch(r"rnn\.weight_hh_l(\d+)", k)] if m)
    if not layers or layers != list(range(len(layers))):
        raise ValueError(f"no rnn.weight_hh_l0 .. l{{L-1}} in the state dict (found layers {layers})")
    L = len(layers)
    names = ["input_embedding.weight", "output_linear.bias"] + [f"rnn.{p}_l{k}" for k in range(L) for p in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
    if not tie_weights or "output_linear.weight" in sd:
        names.append("output_linear.weight")
    missing = [n for n in names if n not in sd]
    if missing:
        raise ValueError(f"the state dict lacks {missing}")
    out = {n: _np(sd[n]) for n in names}
    if tie_weights and "output_linear.weight" in out:
        if out["output_linear.weight"].shape != out["input_embedding.weight"].shape or not np.array_equal(out["output_linear.weight"], out["input_embedding.weight"]):
            raise ValueError("tie_weights: output_linear.weight is not the embedding")
    write_rnn_lm(path, out, L, sos_id, eos_id, tie_weights)
    V, E = out["input_embedding.weight"].shape
    return dict(vocab_size=int(V), embedding_dim=int(E), hidden_dim=int(out["rnn.weight_hh_l0"].shape[1]), num_layers=L)


def main(argv=None) -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("checkpoint")
    ap.add_argument("out")
    ap.add_argument("--sos-id", type=int, default=1)
    ap.add_argument("--eos-id", type=int, default=1)
    ap.add_argument("--tie-weights", action="store_true")
    a = ap.parse_args(argv)
    import torch

    sd = torch.load(a.checkpoint, map_location="cpu")
    print(import_state_dict(sd, a.out, a.sos_id, a.eos_id, a.tie_weights))


if __name__ == "__main__":
    main()
