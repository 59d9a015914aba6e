"""ctypes binding of include/k2hip.h.

Class and method names follow the reference's host API so that the parity tests
read like the reference's own call sites:

    reference (C#)                                  here
    ---------------------------------------------   ---------------------------------
    new OfflineRecognizer(enc, dec, joiner, tok)    OfflineRecognizer(weights_path)
    recognizer.CreateOfflineStream()                recognizer.create_offline_stream()
    stream.AddSamples(float[])                      stream.add_samples(np.ndarray)
    recognizer.GetResults(List<OfflineStream>)      recognizer.get_results([streams])
    recognizer.GetResult(stream)                    recognizer.get_result(stream)
    IOfflineProj.EncoderProj / DecoderProj / ...    Model.encoder_proj / decoder_proj / joiner_proj

(K2TransducerAsr/OfflineRecognizer.cs:27-91, OfflineStream.cs:43-57,
IOfflineProj.cs:43-47.)  All arithmetic happens inside libk2hip.so on the GPU.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import weakref
from typing import List, Optional, Sequence

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(_HERE, "libk2hip.so")
_CSRC = os.path.join(_HERE, "csrc")


class K2HipError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"k2hip error {code}: {msg}")
        self.code = code


def library_path() -> str:
    return _SO


def build_library(force: bool = False) -> str:
    """Compile csrc/*.hip for gfx950 into libk2hip.so (in-tree)."""
    if force:
        subprocess.check_call(["make", "-C", _CSRC, "-s", "clean"])
    subprocess.check_call(["make", "-C", _CSRC, "-s", "-j8"])
    return _SO


class TimingStruct(C.Structure):
    _fields_ = [
        ("total_ms", C.c_float), ("fbank_ms", C.c_float), ("pad_ms", C.c_float), ("encoder_ms", C.c_float),
        ("greedy_ms", C.c_float), ("d2h_ms", C.c_float), ("gemm_ms", C.c_float), ("gemm_launches", C.c_int32),
        ("gemm_flops", C.c_double), ("total_flops", C.c_double),
    ]


class InfoStruct(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("vocab_size", "context_size", "joiner_dim", "feature_dim", "sample_rate",
                                         "num_stacks", "device", "reserved")]


_lib = None
fp = C.POINTER(C.c_float)
ip = C.POINTER(C.c_int32)
lp = C.POINTER(C.c_int64)


def load_library():
    """Load libk2hip.so.  No fallback: a missing library is an error."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_SO):
        raise K2HipError(-2, f"{_SO} is not built; run `python -c 'import __graft_entry__ as g; g.build()'` "
                             "(there is no CPU fallback for this package)")
    L = C.CDLL(_SO)
    vp = C.c_void_p
    L.k2hip_version.restype = C.c_char_p
    L.k2hip_last_error.restype = C.c_char_p
    L.k2hip_device_count.restype = C.c_int32
    L.k2hip_model_create.argtypes = [C.c_char_p, C.c_char_p, C.c_int32, C.POINTER(vp)]
    L.k2hip_model_destroy.argtypes = [vp]
    L.k2hip_model_get_info.argtypes = [vp, C.POINTER(InfoStruct)]
    L.k2hip_model_meta.argtypes = [vp, C.c_char_p, C.c_char_p, C.c_int32]
    L.k2hip_set_instrument.argtypes = [vp, C.c_int32]
    L.k2hip_get_timing.argtypes = [vp, C.POINTER(TimingStruct)]
    L.k2hip_fbank_num_frames.restype = C.c_int64
    L.k2hip_fbank_num_frames.argtypes = [vp, C.c_int64]
    L.k2hip_fbank.argtypes = [vp, fp, C.c_int64, fp, C.c_int64, lp]
    L.k2hip_pad_sequence.argtypes = [vp, C.POINTER(fp), lp, C.c_int32, C.c_int32, fp, C.c_int64, lp]
    L.k2hip_encoder_out_frames.argtypes = [vp, C.c_int32]
    L.k2hip_offline_encoder.argtypes = [vp, fp, lp, C.c_int32, C.c_int32, fp, C.c_int64, lp, ip]
    L.k2hip_offline_encoder_tap.argtypes = [vp, fp, C.c_int32, C.c_int32, C.c_int32, fp, C.c_int64, lp]
    L.k2hip_decoder.argtypes = [vp, lp, C.c_int32, fp]
    L.k2hip_joiner.argtypes = [vp, fp, fp, C.c_int32, fp]
    L.k2hip_greedy_batch.argtypes = [vp, fp, C.c_int32, C.c_int32, lp, ip, ip, C.c_int32]
    L.k2hip_beam_search.argtypes = [vp, fp, C.c_int32, C.c_int32, C.c_int32, lp, ip, ip, C.c_int32, fp]
    L.k2hip_set_decoding_method.argtypes = [vp, C.c_char_p, C.c_int32]
    L.k2hip_last_scores.argtypes = [vp, fp, C.c_int32]
    L.k2hip_greedy_single.argtypes = [vp, fp, C.c_int32, lp, ip, ip, C.c_int32]
    L.k2hip_offline_greedy.argtypes = [vp, C.POINTER(fp), lp, C.c_int32, lp, ip, ip, C.c_int32]
    L.k2hip_offline_greedy_single.argtypes = [vp, fp, C.c_int64, lp, ip, ip, C.c_int32]
    L.k2hip_offline_greedy_from_samples.argtypes = [vp, C.POINTER(fp), lp, C.c_int32, lp, ip, ip, C.c_int32]
    L.k2hip_offline_greedy_from_samples_dev.argtypes = [vp, vp, C.c_int64, C.c_int32, lp, ip, ip, C.c_int32]
    L.k2hip_offline_submit_samples_dev.argtypes = [vp, vp, C.c_int64, C.c_int32, C.c_int32, ip]
    L.k2hip_offline_wait.argtypes = [vp, C.c_int32, lp, ip, ip]
    L.k2hip_offline_submit_samples.argtypes = [vp, fp, C.c_int64, C.c_int32, C.c_int32, ip]
    L.k2hip_host_alloc.argtypes = [vp, C.c_int64, C.POINTER(vp)]
    L.k2hip_host_free.argtypes = [vp, vp]
    L.k2hip_device_alloc.argtypes = [vp, C.c_int64, C.POINTER(vp)]
    L.k2hip_device_free.argtypes = [vp, vp]
    L.k2hip_device_upload.argtypes = [vp, vp, vp, C.c_int64]
    L.k2hip_synchronize.argtypes = [vp]
    L.k2hip_offline_stream_create.argtypes = [vp, C.POINTER(vp)]
    L.k2hip_offline_stream_destroy.argtypes = [vp]
    L.k2hip_offline_stream_accept_samples.argtypes = [vp, fp, C.c_int64]
    L.k2hip_offline_stream_speech_length.restype = C.c_int64
    L.k2hip_offline_stream_speech_length.argtypes = [vp]
    L.k2hip_offline_stream_get_speech.argtypes = [vp, fp, C.c_int64]
    L.k2hip_offline_recognizer_get_results.argtypes = [vp, C.POINTER(vp), C.c_int32]
    L.k2hip_offline_recognizer_get_result.argtypes = [vp, vp]
    L.k2hip_offline_stream_num_tokens.argtypes = [vp]
    L.k2hip_offline_stream_num_timestamps.argtypes = [vp]
    L.k2hip_offline_stream_get_tokens.argtypes = [vp, lp, C.c_int32]
    L.k2hip_offline_stream_get_timestamps.argtypes = [vp, ip, C.c_int32]
    L.k2hip_resample_num_out.restype = C.c_int64
    L.k2hip_resample_num_out.argtypes = [vp, C.c_int32, C.c_int64]
    L.k2hip_resample.argtypes = [vp, C.c_int32, fp, C.c_int64, fp, C.c_int64, lp]
    L.k2hip_offline_stream_accept_waveform.argtypes = [vp, C.c_int32, fp, C.c_int64]
    L.k2hip_online_stream_accept_waveform.argtypes = [vp, C.c_int32, fp, C.c_int64]
    L.k2hip_online_accept_waveform_batch.argtypes = [vp, C.POINTER(vp), C.c_int32, C.c_int32, C.POINTER(fp), lp]
    _lib = L
    return L


def set_switch(env_name: str, value: int = 1):
    """k2hip_debug_set_switch: flip one development switch (named like its K2HIP_* environment variable) after start-up"""
    L = load_library()
    L.k2hip_debug_set_switch.argtypes = [C.c_char_p, C.c_int32]
    rc = L.k2hip_debug_set_switch(env_name.encode(), int(value))
    if rc != 0:
        raise K2HipError(rc, L.k2hip_last_error().decode())


def _f(a):
    return a.ctypes.data_as(fp)


def _i(a):
    return a.ctypes.data_as(ip)


def _l(a):
    return a.ctypes.data_as(lp)


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


class TokenTable:
    """tokens.txt + the reference's token -> text stage (OfflineRecognizer.DecodeMulti / CheckText, :432-565); host only."""

    def __init__(self, tokens_path: str):
        self._L = load_library()
        self._L.k2hip_tokens_load.argtypes = [C.c_char_p, C.POINTER(C.c_void_p)]
        self._L.k2hip_tokens_destroy.argtypes = [C.c_void_p]
        self._L.k2hip_tokens_size.argtypes = [C.c_void_p]
        self._L.k2hip_decode_text.argtypes = [C.c_void_p, lp, C.c_int32, C.c_int32, C.c_char_p, C.c_int32, ip]
        h = C.c_void_p()
        rc = self._L.k2hip_tokens_load(tokens_path.encode(), C.byref(h))
        if rc != 0:
            raise K2HipError(rc, self._L.k2hip_last_error().decode())
        self._h = h

    def __len__(self):
        return self._L.k2hip_tokens_size(self._h)

    def decode(self, ids, online: bool = False) -> str:
        a = np.ascontiguousarray(ids, dtype=np.int64)
        n = C.c_int32()
        rc = self._L.k2hip_decode_text(self._h, _l(a), a.size, int(online), None, 0, C.byref(n))
        if rc != 0:
            raise K2HipError(rc, self._L.k2hip_last_error().decode())
        buf = C.create_string_buffer(n.value + 1)
        rc = self._L.k2hip_decode_text(self._h, _l(a), a.size, int(online), buf, n.value + 1, C.byref(n))
        if rc != 0:
            raise K2HipError(rc, self._L.k2hip_last_error().decode())
        return buf.raw[: n.value].decode("utf-8")

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                self._L.k2hip_tokens_destroy(self._h)
                self._h = None
        except Exception:
            pass


class NgramLm:
    """A back-off n-gram LM over the model's own tokens for shallow fusion in the offline modified beam search (k2hip_ngram_lm_t;
    include/k2hip.h "n-gram LM shallow fusion").  Host only: built, parsed and walked without a GPU.  `entries`: (ids, log_prob,
    backoff) with natural-log float32 weights; NgramLm.BOS / EOS / UNK stand for <s>, </s> and the LM's own <unk>.  NgramLm.load
    reads a text ARPA file whose words are the token strings of a TokenTable."""
    BOS, EOS, UNK = -1, -2, -3

    def _bind(self):
        self._h = None
        self._L = L = load_library()
        L.k2hip_ngram_lm_create.argtypes = [lp, ip, fp, fp, C.c_int64, C.c_int32, C.POINTER(C.c_void_p)]
        L.k2hip_ngram_lm_load.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_void_p)]
        L.k2hip_ngram_lm_destroy.argtypes = [C.c_void_p]
        for f in ("order", "num_states", "num_arcs", "start_state"):
            getattr(L, "k2hip_ngram_lm_" + f).argtypes = [C.c_void_p]
        L.k2hip_ngram_lm_num_arcs.restype = C.c_int64
        L.k2hip_ngram_lm_step.argtypes = [C.c_void_p, C.c_int32, C.c_int64, ip, fp]
        return L

    def __init__(self, entries, vocab_size: int):
        L = self._bind()
        entries = [(list(e[0]), e[1], e[2] if len(e) > 2 else 0.0) for e in entries]
        ids = np.ascontiguousarray([t for e in entries for t in e[0]] or [0], dtype=np.int64)
        orders = np.ascontiguousarray([len(e[0]) for e in entries] or [0], dtype=np.int32)
        lps = np.ascontiguousarray([e[1] for e in entries] or [0], dtype=np.float32)
        bos = np.ascontiguousarray([e[2] for e in entries] or [0], dtype=np.float32)
        h = C.c_void_p()
        rc = L.k2hip_ngram_lm_create(_l(ids), _i(orders), _f(lps), _f(bos), len(entries), int(vocab_size), C.byref(h))
        if rc != 0:
            raise K2HipError(rc, L.k2hip_last_error().decode())
        self._h = h

    @classmethod
    def load(cls, tokens: "TokenTable", path: str) -> "NgramLm":
        lm = cls.__new__(cls)
        L = lm._bind()
        h = C.c_void_p()
        rc = L.k2hip_ngram_lm_load(tokens._h, path.encode(), C.byref(h))
        if rc != 0:
            raise K2HipError(rc, L.k2hip_last_error().decode())
        lm._h = h
        return lm

    @property
    def order(self) -> int:
        return self._L.k2hip_ngram_lm_order(self._h)

    @property
    def num_states(self) -> int:
        return self._L.k2hip_ngram_lm_num_states(self._h)

    @property
    def num_arcs(self) -> int:
        return self._L.k2hip_ngram_lm_num_arcs(self._h)

    @property
    def start_state(self) -> int:
        return self._L.k2hip_ngram_lm_start_state(self._h)

    def step(self, state: int, token: int):
        """(next state, unscaled log-prob) of a hypothesis in `state` that appends `token`"""
        n, b = C.c_int32(), C.c_float()
        rc = self._L.k2hip_ngram_lm_step(self._h, state, token, C.byref(n), C.byref(b))
        if rc != 0:
            raise K2HipError(rc, self._L.k2hip_last_error().decode())
        return n.value, np.float32(b.value)

    def close(self):
        if getattr(self, "_h", None):
            self._L.k2hip_ngram_lm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _bind_rnn_lm(L):
    if getattr(L, "_rnn_lm_bound", False):
        return
    vp = C.c_void_p
    L.k2hip_rnn_lm_load.argtypes = [C.c_char_p, C.POINTER(vp)]
    L.k2hip_rnn_lm_destroy.argtypes = [vp]
    for f in ("vocab_size", "embedding_dim", "hidden_dim", "num_layers", "sos_id", "eos_id"):
        getattr(L, "k2hip_rnn_lm_" + f).argtypes = [vp]
    L.k2hip_rnn_lm_score_host.argtypes = [vp, lp, lp, C.c_int32, C.c_int32, fp, fp]
    L.k2hip_set_rnn_lm.argtypes = [vp, vp, C.c_float]
    L.k2hip_rnn_lm_score.argtypes = [vp, lp, lp, C.c_int32, C.c_int32, fp, fp]
    L.k2hip_offline_stream_get_alternative_lm_score.argtypes = [vp, C.c_int32, fp]
    L.k2hip_debug_rnn_lm_plan.argtypes = [lp, C.c_int32, C.c_int32, C.c_int32, C.c_int64, ip, ip, lp, ip, C.c_int32, ip, ip]
    L.k2hip_debug_rnn_lm_stats.argtypes = [vp, lp, ip]
    L.k2hip_debug_rnn_lm_timing.argtypes = [vp, C.c_int32, C.POINTER(C.c_double)]
    L.k2hip_debug_rnn_lm_step_bench.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, fp, fp]
    L.k2hip_set_rnn_lm_fusion.argtypes = [vp, C.c_int32]
    L.k2hip_debug_rnn_lm_fusion_stats.argtypes = [vp, lp, lp, lp]
    L.k2hip_debug_nlm_advance_bench.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, fp]
    L.k2hip_set_rnn_lm_stream_fusion.argtypes = [vp, C.c_int32]
    L.k2hip_debug_rnn_lm_stream_fusion_stats.argtypes = [vp, lp, lp, lp]
    L._rnn_lm_bound = True


def _pack_hyps(hyps):
    """token-id lists -> (tokens int64, offsets int64 [Hn + 1])"""
    hyps = [np.ascontiguousarray(h, dtype=np.int64).reshape(-1) for h in hyps]
    off = np.zeros(len(hyps) + 1, np.int64)
    if hyps:
        off[1:] = np.cumsum([h.size for h in hyps])
    tok = np.concatenate(hyps + [np.zeros(0, np.int64)]) if hyps else np.zeros(0, np.int64)
    return np.ascontiguousarray(tok if tok.size else np.zeros(1, np.int64)), off


def _rnn_lm_scores(call, handle, hyps, with_eos):
    """(totals [Hn], [token log-probs of hypothesis i]) through k2hip_rnn_lm_score_host / k2hip_rnn_lm_score"""
    tok, off = _pack_hyps(hyps)
    Hn = len(off) - 1
    P = np.diff(off) + (1 if with_eos else 0)
    tlp, tot = np.zeros(max(int(P.sum()), 1), np.float32), np.zeros(max(Hn, 1), np.float32)
    rc = call(handle, _l(tok), _l(off), Hn, int(bool(with_eos)), _f(tlp), _f(tot))
    ends = np.cumsum(P)
    return rc, tot[:Hn].copy(), [tlp[e - n: e].copy() for e, n in zip(ends, P)]


def rnn_lm_plan(lengths, with_eos: bool = True, hidden_dim: int = 32, gx_cap_floats: int = 0) -> dict:
    """the host plan of a scoring call over hypotheses of these lengths (k2hip_debug_rnn_lm_plan; no GPU): dict(order, active, base,
    block): csrc/rnn_lm_plan.h"""
    L = load_library()
    _bind_rnn_lm(L)
    off = np.zeros(len(lengths) + 1, np.int64)
    off[1:] = np.cumsum(np.asarray(lengths, np.int64))
    Hn = len(lengths)
    cap = int(max(list(lengths) + [0])) + 1
    order, active = np.zeros(max(Hn, 1), np.int32), np.zeros(cap, np.int32)
    base, block = np.zeros(cap + 1, np.int64), np.zeros(cap + 1, np.int32)
    T, nb = C.c_int32(), C.c_int32()
    rc = L.k2hip_debug_rnn_lm_plan(_l(off), Hn, int(bool(with_eos)), int(hidden_dim), int(gx_cap_floats), _i(order), _i(active), _l(base), _i(block),
                                   cap, C.byref(T), C.byref(nb))
    if rc != 0:
        raise K2HipError(rc, L.k2hip_last_error().decode())
    return dict(order=order[:Hn].tolist(), active=active[: T.value].tolist(), base=base[: T.value + 1].tolist(), block=block[: nb.value + 1].tolist())


class RnnLm:
    """A neural LM for rescoring N-best lists (k2hip_rnn_lm_t; include/k2hip.h "Neural LM rescoring"): icefall's RnnLmModel (embedding,
    multi-layer LSTM, linear, log_softmax) in a .k2w container (synth.write_synthetic_rnn_lm, rnn_lm_import.py).  Host only: loaded,
    checked and scored (score_host: the float32 reference) without a GPU."""

    def __init__(self, path: str):
        self._h = None
        self._L = L = load_library()
        _bind_rnn_lm(L)
        h = C.c_void_p()
        rc = L.k2hip_rnn_lm_load(path.encode(), C.byref(h))
        if rc != 0:
            raise K2HipError(rc, L.k2hip_last_error().decode())
        self._h = h

    vocab_size = property(lambda self: self._L.k2hip_rnn_lm_vocab_size(self._h))
    embedding_dim = property(lambda self: self._L.k2hip_rnn_lm_embedding_dim(self._h))
    hidden_dim = property(lambda self: self._L.k2hip_rnn_lm_hidden_dim(self._h))
    num_layers = property(lambda self: self._L.k2hip_rnn_lm_num_layers(self._h))
    sos_id = property(lambda self: self._L.k2hip_rnn_lm_sos_id(self._h))
    eos_id = property(lambda self: self._L.k2hip_rnn_lm_eos_id(self._h))

    def score_host(self, hyps, with_eos: bool = True):
        """(totals [Hn] float32, [token log-probs of hypothesis i]) of token-id lists by the host reference"""
        rc, tot, tlp = _rnn_lm_scores(self._L.k2hip_rnn_lm_score_host, self._h, hyps, with_eos)
        if rc != 0:
            raise K2HipError(rc, self._L.k2hip_last_error().decode())
        return tot, tlp

    def close(self):
        if getattr(self, "_h", None):
            self._L.k2hip_rnn_lm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Hotwords:
    """The hotword graph of the modified beam search, set per model for the offline search or per stream for the streaming one
    (k2hip_hotwords_t; include/k2hip.h "hotword biasing"): a trie of token-id phrases with Aho-Corasick failure links.  Host only: built and walked without a GPU.  `phrases`: sequences of token
    ids; `score` = the bonus per matched token.  Hotwords.load reads a pre-tokenised text file through a TokenTable."""

    def _bind(self):
        self._h = None
        self._L = L = load_library()
        L.k2hip_hotwords_create.argtypes = [lp, ip, C.c_int32, C.c_float, C.c_int32, C.POINTER(C.c_void_p)]
        L.k2hip_hotwords_load.argtypes = [C.c_void_p, C.c_char_p, C.c_float, C.POINTER(C.c_void_p)]
        L.k2hip_hotwords_destroy.argtypes = [C.c_void_p]
        L.k2hip_hotwords_num_states.argtypes = [C.c_void_p]
        L.k2hip_hotwords_step.argtypes = [C.c_void_p, C.c_int32, C.c_int64, ip, fp]
        L.k2hip_hotwords_pending.argtypes = [C.c_void_p, C.c_int32, fp]
        return L

    def __init__(self, phrases, score: float, vocab_size: int):
        L = self._bind()
        phrases = [list(p) for p in phrases]
        ids = np.ascontiguousarray([t for p in phrases for t in p] or [0], dtype=np.int64)
        lens = np.ascontiguousarray([len(p) for p in phrases] or [0], dtype=np.int32)
        h = C.c_void_p()
        rc = L.k2hip_hotwords_create(_l(ids), _i(lens), len(phrases), float(score), int(vocab_size), C.byref(h))
        if rc != 0:
            raise K2HipError(rc, L.k2hip_last_error().decode())
        self._h = h

    @classmethod
    def load(cls, tokens: "TokenTable", path: str, score: float) -> "Hotwords":
        hw = cls.__new__(cls)
        L = hw._bind()
        h = C.c_void_p()
        rc = L.k2hip_hotwords_load(tokens._h, path.encode(), float(score), C.byref(h))
        if rc != 0:
            raise K2HipError(rc, L.k2hip_last_error().decode())
        hw._h = h
        return hw

    @property
    def num_states(self) -> int:
        return self._L.k2hip_hotwords_num_states(self._h)

    def step(self, state: int, token: int):
        """(next state, bonus) of a hypothesis in `state` that appends `token`"""
        n, b = C.c_int32(), C.c_float()
        rc = self._L.k2hip_hotwords_step(self._h, state, token, C.byref(n), C.byref(b))
        if rc != 0:
            raise K2HipError(rc, self._L.k2hip_last_error().decode())
        return n.value, np.float32(b.value)

    def pending(self, state: int):
        """the bonus an unfinished match in `state` holds (taken back when the search ends)"""
        b = C.c_float()
        rc = self._L.k2hip_hotwords_pending(self._h, state, C.byref(b))
        if rc != 0:
            raise K2HipError(rc, self._L.k2hip_last_error().decode())
        return np.float32(b.value)

    def close(self):
        if getattr(self, "_h", None):
            self._L.k2hip_hotwords_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Keywords:
    """The keyword graph of the transducer keyword spotter (k2hip_keywords_t; include/k2hip.h "Keyword spotting"): a trie of token-id
    keywords, each with a threshold in (0, 1] on the geometric mean of its tokens' probabilities.  Host only: built without a GPU and
    without a model.  `thresholds`: one number for all keywords or one per keyword.  Keywords.load reads a pre-tokenised text file
    through a TokenTable (an optional last field ":0.35" is the line's threshold)."""

    def _bind(self):
        self._h = None
        self._L = L = load_library()
        L.k2hip_keywords_create.argtypes = [lp, ip, fp, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]
        L.k2hip_keywords_load.argtypes = [C.c_void_p, C.c_char_p, C.c_float, C.POINTER(C.c_void_p)]
        L.k2hip_keywords_destroy.argtypes = [C.c_void_p]
        L.k2hip_keywords_num_states.argtypes = [C.c_void_p]
        L.k2hip_keywords_num_keywords.argtypes = [C.c_void_p]
        L.k2hip_debug_keywords_get_tables.argtypes = [C.c_void_p, ip, ip, ip, ip, fp, C.c_int32]
        return L

    def __init__(self, keywords, thresholds, vocab_size: int):
        L = self._bind()
        keywords = [list(k) for k in keywords]
        thr = np.broadcast_to(np.asarray(thresholds, np.float32), (len(keywords),)) if keywords else np.zeros(0, np.float32)
        ids = np.ascontiguousarray([t for k in keywords for t in k] or [0], dtype=np.int64)
        lens = np.ascontiguousarray([len(k) for k in keywords] or [0], dtype=np.int32)
        thr = np.ascontiguousarray(thr if thr.size else [1.0], dtype=np.float32)
        h = C.c_void_p()
        rc = L.k2hip_keywords_create(_l(ids), _i(lens), _f(thr), len(keywords), int(vocab_size), C.byref(h))
        if rc != 0:
            raise K2HipError(rc, L.k2hip_last_error().decode())
        self._h = h

    @classmethod
    def load(cls, tokens: "TokenTable", path: str, threshold: float) -> "Keywords":
        kw = cls.__new__(cls)
        L = kw._bind()
        h = C.c_void_p()
        rc = L.k2hip_keywords_load(tokens._h, path.encode(), float(threshold), C.byref(h))
        if rc != 0:
            raise K2HipError(rc, L.k2hip_last_error().decode())
        kw._h = h
        return kw

    @property
    def num_states(self) -> int:
        return self._L.k2hip_keywords_num_states(self._h)

    @property
    def num_keywords(self) -> int:
        return self._L.k2hip_keywords_num_keywords(self._h)

    def tables(self) -> dict:
        """the trie as the library built it: parent, tok, depth, kw (int32 [S]) and bar (float32 [S])"""
        S = self.num_states
        out = dict(parent=np.zeros(S, np.int32), tok=np.zeros(S, np.int32), depth=np.zeros(S, np.int32), kw=np.zeros(S, np.int32),
                   bar=np.zeros(S, np.float32))
        rc = self._L.k2hip_debug_keywords_get_tables(self._h, _i(out["parent"]), _i(out["tok"]), _i(out["depth"]), _i(out["kw"]), _f(out["bar"]), S)
        if rc != 0:
            raise K2HipError(rc, self._L.k2hip_last_error().decode())
        return out

    def close(self):
        if getattr(self, "_h", None):
            self._L.k2hip_keywords_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _bind_kws(L):
    if getattr(L, "_kws_bound", False):
        return
    L.k2hip_kws_stream_create.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]
    L.k2hip_kws_stream_destroy.argtypes = [C.c_void_p]
    L.k2hip_kws_stream_reset.argtypes = [C.c_void_p]
    L.k2hip_kws_stream_num_frames.argtypes = [C.c_void_p]
    L.k2hip_kws_stream_num_frames.restype = C.c_int64
    L.k2hip_kws_stream_num_events.argtypes = [C.c_void_p]
    L.k2hip_kws_stream_get_events.argtypes = [C.c_void_p, ip, ip, ip, fp, fp, C.c_int32]
    L.k2hip_kws_stream_clear_events.argtypes = [C.c_void_p]
    L.k2hip_kws_search_chunk.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_int32, fp, C.c_int32, ip]
    L.k2hip_debug_kws_stream_get_state.argtypes = [C.c_void_p, fp, ip, C.c_int32]
    L.k2hip_offline_spot_keywords_from_samples.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(fp), lp, C.c_int32, ip, ip, ip, fp, fp, ip, C.c_int32, ip]
    L._kws_bound = True


def _kws_events(k, st, en, sm, sc, n):
    return [dict(keyword=int(k[i]), start=int(st[i]), end=int(en[i]), sum_logp=np.float32(sm[i]), score=np.float32(sc[i])) for i in range(n)]


class KeywordStream:
    """One audio stream watched for the keywords of a graph (k2hip_kws_stream_*; include/k2hip.h "Keyword spotting"): the tokens carried
    across chunks and the events found so far.  The streaming recipe is OnlineProj.encoder_proj followed by
    KeywordStream.search_chunk.  An event is dict(keyword, start, end, sum_logp, score): frames are absolute since creation or reset."""

    def __init__(self, model: "Model", keywords: Keywords):
        self._m = model
        self._L = model._L
        _bind_kws(self._L)
        h = C.c_void_p()
        model._chk(self._L.k2hip_kws_stream_create(model.handle, keywords._h, C.byref(h)))
        self._h = h
        self._S = keywords.num_states
        model._children.add(self)

    def close(self):
        if getattr(self, "_h", None):
            self._L.k2hip_kws_stream_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self):
        self._m._chk(self._L.k2hip_kws_stream_reset(self._h))

    def num_frames(self) -> int:
        return int(self._L.k2hip_kws_stream_num_frames(self._h))

    @staticmethod
    def search_chunk(streams: Sequence["KeywordStream"], enc_out, n_frames=None):
        """continue every stream's search over enc_out [B, Tc, J] (k2hip_kws_search_chunk); n_frames [B]: the frames of each stream
        that count (default all Tc; 0 leaves a stream untouched).  The streams may walk different graphs."""
        m = streams[0]._m
        e = _f32(enc_out)
        B = len(streams)
        if e.ndim != 3 or e.shape[0] != B:
            raise ValueError(f"search_chunk: enc_out {e.shape} for {B} streams")
        nf = None if n_frames is None else np.ascontiguousarray(n_frames, dtype=np.int32)
        arr = (C.c_void_p * B)(*[s._h.value for s in streams])
        m._chk(m._L.k2hip_kws_search_chunk(m.handle, arr, B, _f(e), e.shape[1], None if nf is None else _i(nf)))

    def events(self, clear: bool = False):
        n = self._L.k2hip_kws_stream_num_events(self._h)
        k, st, en = (np.zeros(max(n, 1), np.int32) for _ in range(3))
        sm, sc = (np.zeros(max(n, 1), np.float32) for _ in range(2))
        got = self._L.k2hip_kws_stream_get_events(self._h, _i(k), _i(st), _i(en), _f(sm), _f(sc), n)
        if got < 0:
            raise K2HipError(got, self._L.k2hip_last_error().decode())
        if clear:
            self._m._chk(self._L.k2hip_kws_stream_clear_events(self._h))
        return _kws_events(k, st, en, sm, sc, n)

    def state(self):
        """the carried block (a float32 [S], start int32 [S]) -- the debug header's view, for the chunking tests"""
        a, st = np.zeros(self._S, np.float32), np.zeros(self._S, np.int32)
        self._m._chk(self._L.k2hip_debug_kws_stream_get_state(self._h, _f(a), _i(st), self._S))
        return a, st


def _bind_ctc_kws(L):
    if getattr(L, "_ctc_kws_bound", False):
        return
    L.k2hip_ctc_kws_stream_create.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]
    L.k2hip_ctc_kws_stream_destroy.argtypes = [C.c_void_p]
    L.k2hip_ctc_kws_stream_reset.argtypes = [C.c_void_p]
    L.k2hip_ctc_kws_stream_num_frames.argtypes = [C.c_void_p]
    L.k2hip_ctc_kws_stream_num_frames.restype = C.c_int64
    L.k2hip_ctc_kws_stream_num_events.argtypes = [C.c_void_p]
    L.k2hip_ctc_kws_stream_get_events.argtypes = [C.c_void_p, ip, ip, ip, fp, fp, C.c_int32]
    L.k2hip_ctc_kws_stream_clear_events.argtypes = [C.c_void_p]
    L.k2hip_ctc_kws_search_chunk.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_int32, fp, C.c_int32, ip]
    L.k2hip_debug_ctc_kws_stream_get_state.argtypes = [C.c_void_p, fp, ip, C.c_int32]
    L.k2hip_offline_ctc_spot_keywords_from_samples.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(fp), lp, C.c_int32, ip, ip, ip, fp, fp, ip, C.c_int32,
                                                               ip]
    L._ctc_kws_bound = True


class CtcKeywordStream:
    """One audio stream of a CTC model watched for the keywords of a graph (k2hip_ctc_kws_stream_*; include/k2hip.h "Keyword spotting for
    CTC models"): the cells carried across chunks and the events found so far.  The streaming recipe is OnlineProj.encoder_proj (the
    log-probs of a streaming CTC model) followed by CtcKeywordStream.search_chunk.  An event is dict(keyword, start, end, sum_logp,
    score): frames are absolute since creation or reset."""

    def __init__(self, model: "Model", keywords: Keywords):
        self._m = model
        self._L = model._L
        _bind_ctc_kws(self._L)
        h = C.c_void_p()
        model._chk(self._L.k2hip_ctc_kws_stream_create(model.handle, keywords._h, C.byref(h)))
        self._h = h
        self._S = keywords.num_states
        model._children.add(self)

    def close(self):
        if getattr(self, "_h", None):
            self._L.k2hip_ctc_kws_stream_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self):
        self._m._chk(self._L.k2hip_ctc_kws_stream_reset(self._h))

    def num_frames(self) -> int:
        return int(self._L.k2hip_ctc_kws_stream_num_frames(self._h))

    @staticmethod
    def search_chunk(streams: Sequence["CtcKeywordStream"], log_probs, n_frames=None):
        """continue every stream's search over log_probs [B, Tc, V] (k2hip_ctc_kws_search_chunk); n_frames [B]: the frames of each stream
        that count (default all Tc; 0 leaves a stream untouched).  The streams may walk different graphs."""
        m = streams[0]._m
        e = _f32(log_probs)
        B = len(streams)
        if e.ndim != 3 or e.shape[0] != B or e.shape[2] != m.vocab_size:
            raise ValueError(f"search_chunk: log_probs {e.shape} for {B} streams of vocab_size {m.vocab_size}")
        nf = None if n_frames is None else np.ascontiguousarray(n_frames, dtype=np.int32)
        if nf is not None and nf.shape != (B,):
            raise ValueError(f"search_chunk: n_frames {nf.shape} for {B} streams")
        arr = (C.c_void_p * B)(*[s._h.value for s in streams])
        m._chk(m._L.k2hip_ctc_kws_search_chunk(m.handle, arr, B, _f(e), e.shape[1], None if nf is None else _i(nf)))

    def events(self, clear: bool = False):
        n = self._L.k2hip_ctc_kws_stream_num_events(self._h)
        k, st, en = (np.zeros(max(n, 1), np.int32) for _ in range(3))
        sm, sc = (np.zeros(max(n, 1), np.float32) for _ in range(2))
        got = self._L.k2hip_ctc_kws_stream_get_events(self._h, _i(k), _i(st), _i(en), _f(sm), _f(sc), n)
        if got < 0:
            raise K2HipError(got, self._L.k2hip_last_error().decode())
        if clear:
            self._m._chk(self._L.k2hip_ctc_kws_stream_clear_events(self._h))
        return _kws_events(k, st, en, sm, sc, n)

    def state(self):
        """the carried block (values float32 [2, S], starts int32 [2, S]; plane 0 = n, plane 1 = b) -- the debug header's view, for the
        chunking tests"""
        v, st = np.zeros((2, self._S), np.float32), np.zeros((2, self._S), np.int32)
        self._m._chk(self._L.k2hip_debug_ctc_kws_stream_get_state(self._h, _f(v), _i(st), 2 * self._S))
        return v, st


class VadConfig(C.Structure):
    """k2hip_vad_config (include/k2hip.h "Voice activity detection and long recordings"): everything in fbank frames; the level
    defaults are in natural-log power units and untuned.  VadConfig.from_seconds converts durations."""
    _fields_ = [("band_lo", C.c_int32), ("band_hi", C.c_int32), ("floor_window", C.c_int32), ("rise", C.c_float), ("margin", C.c_float),
                ("abs_floor", C.c_float), ("min_silence", C.c_int32), ("min_speech", C.c_int32), ("speech_pad", C.c_int32),
                ("max_speech", C.c_int32)]

    def copy(self, **changes) -> "VadConfig":
        c = VadConfig.from_buffer_copy(self)
        for k, v in changes.items():
            if k not in dict(self._fields_):
                raise AttributeError(k)
            setattr(c, k, v)
        return c

    def with_seconds(self, frame_shift_s: float = 0.01, **seconds) -> "VadConfig":
        """a copy with the named durations (floor_window, min_silence, min_speech, speech_pad, max_speech) given in seconds"""
        return self.copy(**{k: int(round(v / frame_shift_s)) for k, v in seconds.items()})

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_}


def _bind_vad(L):
    if getattr(L, "_vad_bound", False):
        return
    vp, cp, bp = C.c_void_p, C.POINTER(VadConfig), C.POINTER(C.c_uint8)
    L.k2hip_vad_default_config.argtypes = [vp, cp]
    L.k2hip_vad_stream_create.argtypes = [vp, cp, C.POINTER(vp)]
    for f in ("destroy", "reset", "flush", "is_speech", "num_segments"):
        getattr(L, "k2hip_vad_stream_" + f).argtypes = [vp]
    L.k2hip_vad_stream_num_frames.argtypes = [vp]
    L.k2hip_vad_stream_num_frames.restype = C.c_int64
    L.k2hip_vad_stream_get_segments.argtypes = [vp, lp, lp, ip, C.c_int32]
    L.k2hip_vad_stream_pop_segments.argtypes = [vp, C.c_int32]
    L.k2hip_vad_accept_features_batch.argtypes = [vp, C.POINTER(vp), C.POINTER(fp), lp, C.c_int32]
    L.k2hip_vad_accept_samples_batch.argtypes = [vp, C.POINTER(vp), C.c_int32, C.POINTER(fp), lp, C.c_int32]
    L.k2hip_offline_recognize_long.argtypes = [vp, C.c_int32, fp, C.c_int64, cp, C.c_int32, C.c_int64, C.POINTER(vp)]
    L.k2hip_long_result_num_segments.argtypes = [vp]
    L.k2hip_long_result_get_segment.argtypes = [vp, C.c_int32, lp, lp, ip, ip]
    L.k2hip_long_result_get_tokens.argtypes = [vp, C.c_int32, lp, ip, C.c_int32, ip]
    L.k2hip_long_result_destroy.argtypes = [vp]
    L.k2hip_debug_vad_check_config.argtypes = [cp, C.c_int32]
    L.k2hip_debug_vad_default_config.argtypes = [C.c_int32, C.c_int32, C.c_float, C.c_float, cp]
    L.k2hip_debug_vad_pack.argtypes = [lp, C.c_int32, C.c_int32, C.c_int64, ip]
    L.k2hip_debug_vad_ref_stream_create.argtypes = [C.c_int32, cp, C.POINTER(vp)]
    L.k2hip_debug_vad_ref_push.argtypes = [vp, fp, C.c_int64, fp, fp, bp]
    L.k2hip_debug_vad_taps.argtypes = [vp, C.c_int32, fp, fp, bp, C.c_int64, lp]
    L.k2hip_debug_long_timing.argtypes = [vp, C.POINTER(C.c_double)]
    L._vad_bound = True


class VadStream:
    """One audio stream of the voice activity detector (k2hip_vad_stream_*).  Segments are dict(start, end, forced) in fbank frames,
    numbered from the stream's start, reset or flush; is_speech tells whether a segment is open.  VadStream(None, cfg, num_bins=n)
    is a stream without a model: only ref_push (the float32 host reference, no GPU) feeds it."""

    def __init__(self, model: Optional["Model"], config: Optional[VadConfig] = None, num_bins: Optional[int] = None):
        self._m = model
        self._L = model._L if model is not None else load_library()
        _bind_vad(self._L)
        self.config = (config if config is not None else model.vad_default_config()).copy()
        h = C.c_void_p()
        if model is None:
            self.num_bins = int(num_bins)
            rc = self._L.k2hip_debug_vad_ref_stream_create(self.num_bins, C.byref(self.config), C.byref(h))
        else:
            self.num_bins = model.feature_dim
            rc = self._L.k2hip_vad_stream_create(model.handle, C.byref(self.config), C.byref(h))
        self._chk(rc)
        self._h = h
        if model is not None:
            model._children.add(self)

    def _chk(self, rc):
        if rc != 0:
            raise K2HipError(rc, self._L.k2hip_last_error().decode())

    def close(self):
        if getattr(self, "_h", None):
            self._L.k2hip_vad_stream_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self):
        self._chk(self._L.k2hip_vad_stream_reset(self._h))

    def flush(self):
        """end of audio: an open segment is closed and reported; the stream then starts over at frame 0"""
        self._chk(self._L.k2hip_vad_stream_flush(self._h))

    @property
    def is_speech(self) -> bool:
        return bool(self._L.k2hip_vad_stream_is_speech(self._h))

    @property
    def num_frames(self) -> int:
        return int(self._L.k2hip_vad_stream_num_frames(self._h))

    def accept_features(self, feats):
        self._m.vad_accept_features([self], [feats])

    def accept_waveform(self, sample_rate: int, samples):
        """samples at any rate (fbank, and the resampler where needed, run on the device; the stream carries what is short of a frame)"""
        self._m.vad_accept_samples([self], sample_rate, [samples])

    def segments(self, pop: bool = False):
        n = self._L.k2hip_vad_stream_num_segments(self._h)
        st, en = np.zeros(max(n, 1), np.int64), np.zeros(max(n, 1), np.int64)
        fo = np.zeros(max(n, 1), np.int32)
        self._chk(self._L.k2hip_vad_stream_get_segments(self._h, _l(st), _l(en), _i(fo), n))
        if pop:
            self._chk(self._L.k2hip_vad_stream_pop_segments(self._h, n))
        return [dict(start=int(st[i]), end=int(en[i]), forced=int(fo[i])) for i in range(n)]

    def ref_push(self, feats):
        """the float32 host reference over these rows (k2hip_debug_vad_ref_push): returns the taps (m, n, d)"""
        f = _f32(feats).reshape(-1, self.num_bins)
        n = f.shape[0]
        m, nn, d = np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.uint8)
        self._chk(self._L.k2hip_debug_vad_ref_push(self._h, _f(f), n, _f(m), _f(nn), d.ctypes.data_as(C.POINTER(C.c_uint8))))
        return m, nn, d


class Model:
    """One model replica on one GPU (k2hip_model_t): the IOfflineProj operators."""

    def __init__(self, weights_path: str, device: int = 0, overrides: Optional[str] = None):
        self._L = load_library()
        h = C.c_void_p()
        rc = self._L.k2hip_model_create(weights_path.encode(), overrides.encode() if overrides else None, device, C.byref(h))
        if rc != 0:
            raise K2HipError(rc, self._L.k2hip_last_error().decode())
        self._h = h
        # the live stream objects of this model: their native destroy calls reach into the model (the slot pool, the engine's lock), so
        # close() closes them first -- a stream that outlives its model's handle is then a closed stream, not a dangling pointer
        self._children = weakref.WeakSet()
        info = InfoStruct()
        self._chk(self._L.k2hip_model_get_info(self._h, C.byref(info)))
        self.vocab_size = info.vocab_size
        self.context_size = info.context_size
        self.joiner_dim = info.joiner_dim
        self.encoder_out_dim = info.reserved  # vocab_size for a zipformer2ctc model (log_probs)
        self.feature_dim = info.feature_dim
        self.sample_rate = info.sample_rate
        self.device = info.device
        self.blank_id, self.sos_eos_id, self.unk_id = 0, 1, 2  # OfflineModel.cs:18-20

    def _chk(self, rc):
        if rc != 0:
            raise K2HipError(rc, self._L.k2hip_last_error().decode())

    def close(self):
        if getattr(self, "_h", None):
            for child in list(getattr(self, "_children", ())):
                child.close()
            self._L.k2hip_model_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    def meta(self, key: str) -> str:
        buf = C.create_string_buffer(4096)
        self._chk(self._L.k2hip_model_meta(self._h, key.encode(), buf, 4096))
        return buf.value.decode()

    def set_instrument(self, on: bool):
        self._chk(self._L.k2hip_set_instrument(self._h, int(on)))

    def timing(self) -> dict:
        t = TimingStruct()
        self._chk(self._L.k2hip_get_timing(self._h, C.byref(t)))
        return {n: getattr(t, n) for n, _ in TimingStruct._fields_}

    # ---- F1
    def fbank_num_frames(self, n: int) -> int:
        return self._L.k2hip_fbank_num_frames(self._h, n)

    def fbank(self, samples) -> np.ndarray:
        s = _f32(samples).reshape(-1)
        nf = max(self.fbank_num_frames(s.size), 0)
        out = np.empty((nf, self.feature_dim), np.float32)
        got = C.c_int64()
        self._chk(self._L.k2hip_fbank(self._h, _f(s), s.size, _f(out), nf, C.byref(got)))
        return out[: got.value]

    # ---- input at other sample rates (include/k2hip.h "Input at other sample rates")
    def resample_num_out(self, in_rate: int, n_in_total: int) -> int:
        """samples at the model's rate that n_in_total samples at in_rate give in all (no flush: the last fraction of a millisecond is
        withheld)"""
        n = self._L.k2hip_resample_num_out(self._h, int(in_rate), int(n_in_total))
        if n < 0:
            raise K2HipError(-1, self._L.k2hip_last_error().decode())
        return int(n)

    def resample(self, samples, in_rate: int) -> np.ndarray:
        """one signal at in_rate converted to the model's rate on the device, in one call"""
        s = _f32(samples).reshape(-1)
        out = np.empty(self.resample_num_out(in_rate, s.size), np.float32)
        got = C.c_int64()
        self._chk(self._L.k2hip_resample(self._h, int(in_rate), _f(s), s.size, _f(out), out.size, C.byref(got)))
        return out[: got.value]

    # ---- voice activity detection and long recordings (include/k2hip.h "Voice activity detection and long recordings")
    def vad_default_config(self) -> VadConfig:
        """the defaults for this model's filterbank: the mel bins centred in [300, 3500] Hz; the levels are untuned"""
        _bind_vad(self._L)
        cfg = VadConfig()
        self._chk(self._L.k2hip_vad_default_config(self._h, C.byref(cfg)))
        return cfg

    def vad_accept_features(self, streams: Sequence["VadStream"], feats: Sequence[np.ndarray]):
        """feats[b] [n_b, feature_dim] for streams[b], all streams in one batched call on the device (0 rows leave a stream untouched)"""
        _bind_vad(self._L)
        B = len(streams)
        fs = [_f32(f).reshape(-1, self.feature_dim) for f in feats]
        if len(fs) != B:
            raise ValueError(f"vad_accept_features: {len(fs)} feature matrices for {B} streams")
        arr = (C.c_void_p * B)(*[s._h.value for s in streams])
        ptrs = (fp * B)(*[_f(f) for f in fs])
        n = np.array([f.shape[0] for f in fs], np.int64)
        self._chk(self._L.k2hip_vad_accept_features_batch(self._h, arr, ptrs, _l(n), B))

    def vad_accept_samples(self, streams: Sequence["VadStream"], sample_rate: int, samples: Sequence[np.ndarray]):
        """samples[b] at sample_rate for streams[b]; fbank runs on the device and the features stay there"""
        _bind_vad(self._L)
        B = len(streams)
        ss = [_f32(s).reshape(-1) for s in samples]
        if len(ss) != B:
            raise ValueError(f"vad_accept_samples: {len(ss)} signals for {B} streams")
        arr = (C.c_void_p * B)(*[s._h.value for s in streams])
        ptrs = (fp * B)(*[_f(s) for s in ss])
        n = np.array([s.size for s in ss], np.int64)
        self._chk(self._L.k2hip_vad_accept_samples_batch(self._h, arr, int(sample_rate), ptrs, _l(n), B))

    def vad_taps(self, b: int = 0):
        """the taps (m, n, d) of stream b's frames in the model's last VAD call (the debug header's view)"""
        _bind_vad(self._L)
        cnt = C.c_int64()
        rc = self._L.k2hip_debug_vad_taps(self._h, b, None, None, None, 0, C.byref(cnt))
        if rc != 0 and cnt.value == 0:
            self._chk(rc)
        m, n, d = np.zeros(cnt.value, np.float32), np.zeros(cnt.value, np.float32), np.zeros(cnt.value, np.uint8)
        if cnt.value:
            self._chk(self._L.k2hip_debug_vad_taps(self._h, b, _f(m), _f(n), d.ctypes.data_as(C.POINTER(C.c_uint8)), cnt.value, C.byref(cnt)))
        return m, n, d

    def recognize_long(self, samples, sample_rate: Optional[int] = None, config: Optional[VadConfig] = None, max_batch: int = 32,
                       max_batch_frames: int = 32000):
        """one long recording: fbank over all of it on the device, the detector, the segments decoded in batches by the model's current
        offline search (k2hip_offline_recognize_long).  Returns a list of dict(start, end, forced, batch, tokens, timestamps): start /
        end in fbank frames of the recording, timestamps in encoder frames of the segment."""
        _bind_vad(self._L)
        s = _f32(samples).reshape(-1)
        h = C.c_void_p()
        self._chk(self._L.k2hip_offline_recognize_long(self._h, int(sample_rate or self.sample_rate), _f(s), s.size,
                                                       C.byref(config) if config is not None else None, int(max_batch), int(max_batch_frames),
                                                       C.byref(h)))
        try:
            out = []
            for i in range(self._L.k2hip_long_result_num_segments(h)):
                st, en, fo, ba, n = C.c_int64(), C.c_int64(), C.c_int32(), C.c_int32(), C.c_int32()
                self._chk(self._L.k2hip_long_result_get_segment(h, i, C.byref(st), C.byref(en), C.byref(fo), C.byref(ba)))
                rc = self._L.k2hip_long_result_get_tokens(h, i, None, None, 0, C.byref(n))
                if rc != 0 and n.value == 0:
                    self._chk(rc)
                tok, ts = np.zeros(max(n.value, 1), np.int64), np.zeros(max(n.value, 1), np.int32)
                self._chk(self._L.k2hip_long_result_get_tokens(h, i, _l(tok), _i(ts), n.value, C.byref(n)))
                out.append(dict(start=st.value, end=en.value, forced=fo.value, batch=ba.value, tokens=tok[: n.value].tolist(),
                                timestamps=ts[: n.value].tolist()))
            return out
        finally:
            self._L.k2hip_long_result_destroy(h)

    def long_timing(self) -> dict:
        """host milliseconds of the last recognize_long by leg"""
        _bind_vad(self._L)
        ms = (C.c_double * 3)()
        self._chk(self._L.k2hip_debug_long_timing(self._h, ms))
        return dict(fbank_ms=ms[0], vad_ms=ms[1], batches_ms=ms[2])

    # ---- neural LM rescoring (include/k2hip.h "Neural LM rescoring")
    def set_rnn_lm(self, lm: Optional["RnnLm"] = None, scale: float = 0.0):
        """k2hip_set_rnn_lm: attach the neural LM (None clears).  With scale > 0 and set_nbest(n > 1), get_results rescores every
        stream's N-best list and re-orders it; with n = 1 there is nothing to rescore and the LM changes nothing."""
        _bind_rnn_lm(self._L)
        self._chk(self._L.k2hip_set_rnn_lm(self._h, lm._h if lm is not None else None, float(scale)))

    def rnn_lm_score(self, hyps, with_eos: bool = True):
        """(totals [Hn] float32, [token log-probs of hypothesis i]) of token-id lists by the attached LM, on the device, in the
        caller's order (k2hip_rnn_lm_score)"""
        _bind_rnn_lm(self._L)
        rc, tot, tlp = _rnn_lm_scores(self._L.k2hip_rnn_lm_score, self._h, hyps, with_eos)
        self._chk(rc)
        return tot, tlp

    def rnn_lm_stats(self) -> dict:
        """scoring calls that reached the device, and the time blocks of the last one (the debug header's view)"""
        _bind_rnn_lm(self._L)
        n, b = C.c_int64(), C.c_int32()
        self._chk(self._L.k2hip_debug_rnn_lm_stats(self._h, C.byref(n), C.byref(b)))
        return dict(device_calls=n.value, last_blocks=b.value)

    def rnn_lm_timing(self, on: bool = True) -> dict:
        """switch the leg timing of the scoring calls; returns the last call's milliseconds by leg"""
        _bind_rnn_lm(self._L)
        ms = (C.c_double * 4)()
        self._chk(self._L.k2hip_debug_rnn_lm_timing(self._h, int(on), ms))
        return dict(embed_ms=ms[0], gx_ms=ms[1], steps_ms=ms[2], score_ms=ms[3])

    def set_rnn_lm_fusion(self, on: bool = True):
        """k2hip_set_rnn_lm_fusion: with an LM of scale > 0 attached, the offline modified beam search adds the LM's term to every
        appended token DURING the search (shallow fusion) and get_results no longer rescores (include/k2hip.h "Neural LM shallow
        fusion")."""
        _bind_rnn_lm(self._L)
        self._chk(self._L.k2hip_set_rnn_lm_fusion(self._h, int(bool(on))))

    def rnn_lm_fusion_stats(self) -> dict:
        """fused searches enqueued by the process; per-layer LM launches of this model's LM that swept their weights / only moved state"""
        _bind_rnn_lm(self._L)
        n, s, i = C.c_int64(), C.c_int64(), C.c_int64()
        self._chk(self._L.k2hip_debug_rnn_lm_fusion_stats(self._h, C.byref(n), C.byref(s), C.byref(i)))
        return dict(searches=n.value, swept=s.value, idle=i.value)

    def set_rnn_lm_stream_fusion(self, on: bool = True):
        """k2hip_set_rnn_lm_stream_fusion: with an LM of scale > 0 attached, the STREAMING modified beam search (BeamStream chunks,
        OnlineRecognizer under modified_beam_search) adds the LM's term during the search and carries every hypothesis' LM state from
        chunk to chunk (include/k2hip.h "Neural LM shallow fusion in the streaming modified beam search").  A switch of its own: the
        offline one (set_rnn_lm_fusion) does not reach streaming entries."""
        _bind_rnn_lm(self._L)
        self._chk(self._L.k2hip_set_rnn_lm_stream_fusion(self._h, int(bool(on))))

    def rnn_lm_stream_fusion_stats(self) -> dict:
        """fused chunk calls enqueued by the process; state blocks this model's streams hold; bytes of the model's block pool"""
        _bind_rnn_lm(self._L)
        n, b, p = C.c_int64(), C.c_int64(), C.c_int64()
        self._chk(self._L.k2hip_debug_rnn_lm_stream_fusion_stats(self._h, C.byref(n), C.byref(b), C.byref(p)))
        return dict(chunk_calls=n.value, live_blocks=b.value, pool_bytes=p.value)

    def nlm_advance_bench(self, rows: int, hidden_dim: int, iters: int = 200) -> float:
        """milliseconds per k_nlm_advance launch (k2hip_debug_nlm_advance_bench)"""
        _bind_rnn_lm(self._L)
        ms = C.c_float()
        self._chk(self._L.k2hip_debug_nlm_advance_bench(self._h, int(rows), int(hidden_dim), int(iters), C.byref(ms)))
        return float(ms.value)

    def rnn_lm_step_bench(self, rows: int, hidden_dim: int, iters: int = 200) -> dict:
        """milliseconds per recurrent step: the fused kernel, and the step composed from the GEMM launcher and the cell kernel"""
        _bind_rnn_lm(self._L)
        a, b = C.c_float(), C.c_float()
        self._chk(self._L.k2hip_debug_rnn_lm_step_bench(self._h, int(rows), int(hidden_dim), int(iters), C.byref(a), C.byref(b)))
        return dict(fused_ms=a.value, composed_ms=b.value)

    # ---- F3
    def pad_sequence(self, feats: Sequence[np.ndarray], tail_frames: int = 19) -> np.ndarray:
        fs = [_f32(f).reshape(-1) for f in feats]
        B = len(fs)
        ptrs = (fp * B)(*[_f(f) for f in fs])
        n = np.array([f.size for f in fs], np.int64)
        L = int(n.max()) + 80 * tail_frames
        out = np.empty((B, L), np.float32)
        got = C.c_int64()
        self._chk(self._L.k2hip_pad_sequence(self._h, ptrs, _l(n), B, tail_frames, _f(out), out.size, C.byref(got)))
        assert got.value == L
        return out

    # ---- F4-F6: IOfflineProj
    def encoder_out_frames(self, T: int) -> int:
        return self._L.k2hip_encoder_out_frames(self._h, T)

    def encoder_proj(self, x) -> np.ndarray:
        x = _f32(x)
        B, T, _ = x.shape
        tp = max(self.encoder_out_frames(T), 0)
        out = np.empty((B, tp, self.encoder_out_dim), np.float32)
        lens = np.zeros(B, np.int64)
        xl = np.full(B, T, np.int64)
        got = C.c_int32()
        self._chk(self._L.k2hip_offline_encoder(self._h, _f(x), _l(xl), B, T, _f(out), out.size, _l(lens), C.byref(got)))
        return out

    def encoder_tap(self, x, tap: int) -> np.ndarray:
        x = _f32(x)
        B, T, _ = x.shape
        buf = np.empty(B * T * 1024, np.float32)
        n = C.c_int64()
        self._chk(self._L.k2hip_offline_encoder_tap(self._h, _f(x), B, T, tap, _f(buf), buf.size, C.byref(n)))
        return buf[: n.value].reshape(B, -1).copy()

    def decoder_proj(self, y=None, N: Optional[int] = None) -> np.ndarray:
        if y is None:
            out = np.empty((N, self.joiner_dim), np.float32)
            self._chk(self._L.k2hip_decoder(self._h, None, N, _f(out)))
            return out
        y = np.ascontiguousarray(y, dtype=np.int64).reshape(-1, self.context_size)
        out = np.empty((y.shape[0], self.joiner_dim), np.float32)
        self._chk(self._L.k2hip_decoder(self._h, _l(y), y.shape[0], _f(out)))
        return out

    def joiner_proj(self, enc, dec) -> np.ndarray:
        enc = _f32(enc).reshape(-1, self.joiner_dim)
        dec = _f32(dec).reshape(-1, self.joiner_dim)
        out = np.empty((enc.shape[0], self.vocab_size), np.float32)
        self._chk(self._L.k2hip_joiner(self._h, _f(enc), _f(dec), enc.shape[0], _f(out)))
        return out

    # ---- F7
    def _unpack(self, tok, ts, n):
        return [(tok[b, : n[b]].tolist(), ts[b, : n[b]].tolist()) for b in range(tok.shape[0])]

    def greedy_batch(self, enc_out):
        e = _f32(enc_out)
        B, Tp, _ = e.shape
        tok = np.zeros((B, Tp), np.int64)
        ts = np.zeros((B, Tp), np.int32)
        n = np.zeros(B, np.int32)
        self._chk(self._L.k2hip_greedy_batch(self._h, _f(e), B, Tp, _l(tok), _i(ts), _i(n), Tp))
        return self._unpack(tok, ts, n)

    def ctc_greedy(self, log_probs, frame_offsets=None, num_trailing_blank=None):
        """ForwardBatchGreedySearchCTC over host log_probs [B,T',V] (k2hip_ctc_greedy)"""
        e = _f32(log_probs)
        B, Tp, _ = e.shape
        tok = np.zeros((B, Tp), np.int64)
        ts = np.zeros((B, Tp), np.int32)
        n = np.zeros(B, np.int32)
        fo = np.zeros(B, np.int32) if frame_offsets is None else np.ascontiguousarray(frame_offsets, dtype=np.int32)
        tb = np.zeros(B, np.int32) if num_trailing_blank is None else np.ascontiguousarray(num_trailing_blank, dtype=np.int32).copy()
        self._L.k2hip_ctc_greedy.argtypes = [C.c_void_p, fp, C.c_int32, C.c_int32, ip, lp, ip, ip, C.c_int32, ip]
        self._chk(self._L.k2hip_ctc_greedy(self._h, _f(e), B, Tp, _i(fo), _l(tok), _i(ts), _i(n), Tp, _i(tb)))
        return self._unpack(tok, ts, n), tb

    def ctc_prefix_beam_search(self, log_probs, beam: int = 4, n_frames=None, nbest: Optional[int] = None, want_scores: bool = False,
                               want_token_log_probs: bool = False, max_tokens: Optional[int] = None):
        """k2hip_ctc_prefix_beam_search over host log_probs [R,T',V] (what the encoder entries of a CTC model return); n_frames [R]: the
        frames of each row that count (default: all T').  With nbest = N: per row a list of up to N alternatives in rank order, each a
        dict(tokens, timestamps, token_log_probs, score); with want_token_log_probs alone the best one's dict per row; otherwise the
        (tokens, timestamps) pairs of ctc_greedy, and the scores [R] behind them with want_scores."""
        x = _f32(log_probs)
        R, Tp, _ = x.shape
        N = 1 if nbest is None else nbest
        M, mt = max(N, 1), Tp if max_tokens is None else max_tokens
        tok = np.zeros((R, M, max(mt, 1)), np.int64)
        ts = np.zeros((R, M, max(mt, 1)), np.int32)
        yp = np.zeros((R, M, max(mt, 1)), np.float32)
        n = np.zeros((R, M), np.int32)
        nh = np.zeros(R, np.int32)
        sc = np.zeros((R, M), np.float32)
        nf = None if n_frames is None else np.ascontiguousarray(n_frames, dtype=np.int32)
        self._L.k2hip_ctc_prefix_beam_search.argtypes = [C.c_void_p, fp, C.c_int32, C.c_int32, ip, C.c_int32, C.c_int32, lp, ip, fp, ip, ip, fp,
                                                         C.c_int32]
        self._chk(self._L.k2hip_ctc_prefix_beam_search(self._h, _f(x), R, Tp, None if nf is None else _i(nf), beam, N, _l(tok), _i(ts), _f(yp),
                                                       _i(n), _i(nh), _f(sc), mt))
        out = [[dict(tokens=tok[r, i, : n[r, i]].tolist(), timestamps=ts[r, i, : n[r, i]].tolist(), token_log_probs=yp[r, i, : n[r, i]].copy(),
                     score=float(sc[r, i])) for i in range(nh[r])] for r in range(R)]
        if nbest is not None:
            return out
        if want_token_log_probs:
            return [alts[0] for alts in out]
        res = [(alts[0]["tokens"], alts[0]["timestamps"]) for alts in out]
        return (res, sc[:, 0].copy()) if want_scores else res

    def set_nbest(self, n: int = 1):
        """k2hip_set_nbest: n > 1 makes the synchronous modified-beam-search entries keep up to n alternatives per stream, each with
        its token log-probs (streams' .alternatives() / .token_log_probs()); 1 = off"""
        self._L.k2hip_set_nbest.argtypes = [C.c_void_p, C.c_int32]
        self._chk(self._L.k2hip_set_nbest(self._h, n))

    def beam_search(self, enc_out, beam: int = 4, want_scores: bool = False, nbest: Optional[int] = None, want_token_log_probs: bool = False):
        """modified beam search over a host encoder_out [B,T',J] (k2hip_beam_search).  With nbest = N and / or want_token_log_probs
        (k2hip_beam_search_nbest): per stream a list of up to N alternatives in pick order (entry 0 = the plain call's result), each a
        dict(tokens, timestamps, token_log_probs, score); without nbest only the best one's dict is returned per stream."""
        e = _f32(enc_out)
        B, Tp, _ = e.shape
        if nbest is not None or want_token_log_probs:
            N = 1 if nbest is None else nbest
            M = max(N, 1)
            tok = np.zeros((B, M, Tp), np.int64)
            ts = np.zeros((B, M, Tp), np.int32)
            yp = np.zeros((B, M, Tp), np.float32)
            n = np.zeros((B, M), np.int32)
            nh = np.zeros(B, np.int32)
            sc = np.zeros((B, M), np.float32)
            self._L.k2hip_beam_search_nbest.argtypes = [C.c_void_p, fp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, lp, ip, fp, ip, ip, fp, C.c_int32]
            self._chk(self._L.k2hip_beam_search_nbest(self._h, _f(e), B, Tp, beam, N, _l(tok), _i(ts), _f(yp), _i(n), _i(nh), _f(sc), Tp))
            out = [[dict(tokens=tok[b, i, : n[b, i]].tolist(), timestamps=ts[b, i, : n[b, i]].tolist(), token_log_probs=yp[b, i, : n[b, i]].copy(),
                         score=float(sc[b, i])) for i in range(nh[b])] for b in range(B)]
            return out if nbest is not None else [alts[0] for alts in out]
        tok = np.zeros((B, Tp), np.int64)
        ts = np.zeros((B, Tp), np.int32)
        n = np.zeros(B, np.int32)
        sc = np.zeros(B, np.float32)
        self._chk(self._L.k2hip_beam_search(self._h, _f(e), B, Tp, beam, _l(tok), _i(ts), _i(n), Tp, _f(sc)))
        res = self._unpack(tok, ts, n)
        return (res, sc) if want_scores else res

    def beam_trace(self):
        """k2hip_debug_beam_trace (include/k2hip_debug.h): the per-frame selection of the last synchronous modified beam search made
        with the switch K2HIP_BEAM_TRACE on -> dict(idx [B,T',beam] flat candidate indexes (slot * V + token) in rank order,
        val [B,T',beam] their scores, n [B,T'] hypotheses surviving the frame, beam)"""
        B, Tp, K = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        self._L.k2hip_debug_beam_trace.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.c_int64] + [C.POINTER(C.c_int32)] * 3
        self._chk(self._L.k2hip_debug_beam_trace(self._h, None, 0, C.byref(B), C.byref(Tp), C.byref(K)))
        tr = np.zeros((B.value, Tp.value, 2 * K.value + 1), np.int32)
        self._chk(self._L.k2hip_debug_beam_trace(self._h, _i(tr), tr.size, C.byref(B), C.byref(Tp), C.byref(K)))
        k = K.value
        return dict(idx=tr[:, :, :k].copy(), val=tr[:, :, k: 2 * k].copy().view(np.float32), n=tr[:, :, 2 * k].copy(), beam=k)

    def set_decoding_method(self, method: str = "greedy_search", beam: int = 4):
        """decodingMethod of the batch entry points (OfflineRecognizer.cs:54-68): greedy_search | modified_beam_search, and for a CTC
        model ctc_prefix_beam_search (no reference counterpart; k2hip.h "CTC prefix beam search with N-best")"""
        self._chk(self._L.k2hip_set_decoding_method(self._h, method.encode(), beam))

    def create_ctc_prefix_stream(self, beam: int, nbest: int = 1) -> "CtcPrefixStream":
        """k2hip_ctc_prefix_stream_create: one stream of the CTC prefix beam search carried across chunks (beam 1..8, nbest 1..beam)"""
        return CtcPrefixStream(self, beam, nbest)

    def ctc_prefix_beam_search_chunk(self, streams, log_probs, n_frames=None):
        """k2hip_ctc_prefix_beam_search_chunk: continue every stream over its next n_frames[b] (None = all Tc) rows of log_probs
        [B, Tc, V].  A failed call leaves every stream as it was."""
        _bind_online(self._L)
        x = _f32(log_probs)
        B = len(streams)
        assert x.ndim == 3 and x.shape[0] == B and x.shape[2] == self.vocab_size, x.shape
        nf = None if n_frames is None else np.ascontiguousarray(n_frames, np.int32)
        assert nf is None or nf.shape == (B,), nf.shape
        arr = (C.c_void_p * B)(*[s._h.value for s in streams])
        self._chk(self._L.k2hip_ctc_prefix_beam_search_chunk(self._h, arr, B, _f(x), x.shape[1], _i(nf) if nf is not None else None))

    def set_ctc_prefix_biasing(self, on: bool = True):
        """k2hip_set_ctc_prefix_biasing: the offline CTC prefix beam search (ctc_prefix_beam_search and the batch entries under that
        decoding method) uses the hotwords and the n-gram LM set on the model; off (the default) it ignores both.  CTC models only."""
        self._L.k2hip_set_ctc_prefix_biasing.argtypes = [C.c_void_p, C.c_int32]
        self._chk(self._L.k2hip_set_ctc_prefix_biasing(self._h, 1 if on else 0))

    def set_hotwords(self, hotwords: Optional["Hotwords"] = None):
        """k2hip_set_hotwords: bias the offline modified beam search towards the graph's phrases; None clears.  The model keeps its own
        copy of the tables."""
        self._L.k2hip_set_hotwords.argtypes = [C.c_void_p, C.c_void_p]
        self._chk(self._L.k2hip_set_hotwords(self._h, hotwords._h if hotwords is not None else None))

    def set_ngram_lm(self, lm: Optional["NgramLm"] = None, scale: float = 0.0):
        """k2hip_set_ngram_lm: shallow fusion of the n-gram LM, weighted by `scale`, in the modified beam search, offline and
        streaming; None clears.  The model keeps its own copy of the scaled tables: lm.close() afterwards is fine."""
        self._L.k2hip_set_ngram_lm.argtypes = [C.c_void_p, C.c_void_p, C.c_float]
        self._chk(self._L.k2hip_set_ngram_lm(self._h, lm._h if lm is not None else None, float(scale)))

    def set_lodr_lm(self, lm: Optional["NgramLm"] = None, scale: float = 0.0):
        """k2hip_set_lodr_lm: LODR, a low-order n-gram LM (usually a bi-gram over the acoustic model's training text) whose score is
        SUBTRACTED wherever the neural LM acts -- the fused offline and streaming modified beam search, and the N-best rescoring of
        get_results.  scale <= 0 (icefall's convention); None or 0 clears.  A slot of its own beside set_ngram_lm's; ignored everywhere
        else (include/k2hip.h "LODR")."""
        self._L.k2hip_set_lodr_lm.argtypes = [C.c_void_p, C.c_void_p, C.c_float]
        self._L.k2hip_set_lodr_lm.restype = C.c_int32
        self._chk(self._L.k2hip_set_lodr_lm(self._h, lm._h if lm is not None else None, float(scale)))

    def gemm_profile(self) -> np.ndarray:
        """[n, 8] rows (M, N, K, batch, act, has_residual, kind, us) of the last instrumented call"""
        n = C.c_int32(0)
        self._L.k2hip_get_gemm_profile.argtypes = [C.c_void_p, fp, C.c_int32, C.POINTER(C.c_int32)]
        self._chk(self._L.k2hip_get_gemm_profile(self._h, None, 0, C.byref(n)))
        rows = np.zeros((max(n.value, 1), 8), np.float32)
        self._chk(self._L.k2hip_get_gemm_profile(self._h, _f(rows), n.value, C.byref(n)))
        return rows[: n.value]

    def last_scores(self, B: int):
        sc = np.zeros(B, np.float32)
        self._chk(self._L.k2hip_last_scores(self._h, _f(sc), B))
        return sc

    def greedy_single(self, enc_out):
        e = _f32(enc_out).reshape(-1, self.joiner_dim)
        Tp = e.shape[0]
        tok = np.zeros((1, Tp), np.int64)
        ts = np.zeros((1, Tp), np.int32)
        n = np.zeros(1, np.int32)
        self._chk(self._L.k2hip_greedy_single(self._h, _f(e), Tp, _l(tok), _i(ts), _i(n), Tp))
        return self._unpack(tok, ts, n)[0]

    def offline_greedy(self, feats: Sequence[np.ndarray]):
        fs = [_f32(f).reshape(-1) for f in feats]
        B = len(fs)
        ptrs = (fp * B)(*[_f(f) for f in fs])
        nfl = np.array([f.size for f in fs], np.int64)
        mt = max(1, self.encoder_out_frames(int(nfl.max()) // self.feature_dim + 19))
        tok = np.zeros((B, mt), np.int64)
        ts = np.zeros((B, mt), np.int32)
        n = np.zeros(B, np.int32)
        self._chk(self._L.k2hip_offline_greedy(self._h, ptrs, _l(nfl), B, _l(tok), _i(ts), _i(n), mt))
        return self._unpack(tok, ts, n)

    def offline_greedy_single(self, feats: np.ndarray):
        f = _f32(feats).reshape(-1)
        mt = max(1, self.encoder_out_frames(f.size // self.feature_dim + 19))
        tok = np.zeros((1, mt), np.int64)
        ts = np.zeros((1, mt), np.int32)
        n = np.zeros(1, np.int32)
        self._chk(self._L.k2hip_offline_greedy_single(self._h, _f(f), f.size, _l(tok), _i(ts), _i(n), mt))
        return self._unpack(tok, ts, n)[0]

    def offline_greedy_from_samples(self, samples: Sequence[np.ndarray]):
        ss = [_f32(s).reshape(-1) for s in samples]
        B = len(ss)
        ptrs = (fp * B)(*[_f(s) for s in ss])
        ns = np.array([s.size for s in ss], np.int64)
        mt = max(1, self.encoder_out_frames(self.fbank_num_frames(int(ns.max())) + 19))
        tok = np.zeros((B, mt), np.int64)
        ts = np.zeros((B, mt), np.int32)
        n = np.zeros(B, np.int32)
        self._chk(self._L.k2hip_offline_greedy_from_samples(self._h, ptrs, _l(ns), B, _l(tok), _i(ts), _i(n), mt))
        return self._unpack(tok, ts, n)

    # ---- forced alignment and full-sum scoring (k2hip.h "Forced alignment and full-sum scoring ...")
    @staticmethod
    def _align_targets(targets):
        tg = [np.ascontiguousarray(t, dtype=np.int64).reshape(-1) for t in targets]
        lens = np.array([t.size for t in tg], np.int32)
        ids = np.concatenate(tg) if tg and int(lens.sum()) else np.zeros(0, np.int64)
        return np.ascontiguousarray(ids, dtype=np.int64), lens

    @staticmethod
    def _align_result(lens, ts, yp, tot, best):
        return [dict(timestamps=ts[b, : lens[b]].tolist(), token_log_probs=yp[b, : lens[b]].copy(), total_logp=float(tot[b]),
                     best_logp=float(best[b])) for b in range(len(lens))]

    def align(self, enc_out, targets, n_frames=None, max_tokens: Optional[int] = None):
        """k2hip_transducer_align over a host encoder_out [B,T',J]: per stream the forced alignment of targets[b] (token ids, neither
        blank nor unk) and its full-sum score -> a list of dict(timestamps, token_log_probs, total_logp, best_logp).  n_frames [B]: the
        frames of each stream that count (default: all T')."""
        e = _f32(enc_out)
        B, Tp, _ = e.shape
        if len(targets) != B:
            raise ValueError(f"align: {len(targets)} targets for {B} streams")
        ids, lens = self._align_targets(targets)
        mt = max(1, int(lens.max())) if max_tokens is None else max_tokens
        nf = None if n_frames is None else np.ascontiguousarray(n_frames, dtype=np.int32)
        ts = np.zeros((B, max(mt, 1)), np.int32)
        yp = np.zeros((B, max(mt, 1)), np.float32)
        tot = np.zeros(B, np.float32)
        best = np.zeros(B, np.float32)
        self._L.k2hip_transducer_align.argtypes = [C.c_void_p, fp, C.c_int32, C.c_int32, ip, lp, ip, ip, fp, fp, fp, C.c_int32]
        self._chk(self._L.k2hip_transducer_align(self._h, _f(e), B, Tp, None if nf is None else _i(nf), _l(ids), _i(lens), _i(ts), _f(yp),
                                                 _f(tot), _f(best), mt))
        return self._align_result(lens, ts, yp, tot, best)

    def align_samples(self, samples: Sequence[np.ndarray], targets, max_tokens: Optional[int] = None):
        """k2hip_offline_align_from_samples: samples -> fbank -> pad -> encoder on the device, then align() over all T' frames of the
        padded batch (the frames the searches decode)"""
        ss = [_f32(s).reshape(-1) for s in samples]
        B = len(ss)
        if len(targets) != B:
            raise ValueError(f"align_samples: {len(targets)} targets for {B} streams")
        ptrs = (fp * B)(*[_f(s) for s in ss])
        ns = np.array([s.size for s in ss], np.int64)
        ids, lens = self._align_targets(targets)
        mt = max(1, int(lens.max())) if max_tokens is None else max_tokens
        ts = np.zeros((B, max(mt, 1)), np.int32)
        yp = np.zeros((B, max(mt, 1)), np.float32)
        tot = np.zeros(B, np.float32)
        best = np.zeros(B, np.float32)
        tp = C.c_int32(0)
        self._L.k2hip_offline_align_from_samples.argtypes = [C.c_void_p, C.POINTER(fp), lp, C.c_int32, lp, ip, ip, fp, fp, fp, C.c_int32, ip]
        self._chk(self._L.k2hip_offline_align_from_samples(self._h, ptrs, _l(ns), B, _l(ids), _i(lens), _i(ts), _f(yp), _f(tot), _f(best), mt,
                                                           C.byref(tp)))
        return self._align_result(lens, ts, yp, tot, best)

    # ---- keyword spotting (k2hip.h "Keyword spotting ...")
    def spot_keywords(self, enc_out, keywords: "Keywords", n_frames=None):
        """fresh keyword streams over a host encoder_out [B,T',J] in one chunk -> per stream the list of events
        dict(keyword, start, end, sum_logp, score)"""
        e = _f32(enc_out)
        streams = [KeywordStream(self, keywords) for _ in range(e.shape[0])]
        try:
            KeywordStream.search_chunk(streams, e, n_frames)
            return [s.events() for s in streams]
        finally:
            for s in streams:
                s.close()

    def spot_keywords_samples(self, samples: Sequence[np.ndarray], keywords: "Keywords", max_events: Optional[int] = None):
        """k2hip_offline_spot_keywords_from_samples: samples -> fbank -> pad -> encoder on the device, then spot_keywords() over all T'
        frames of the padded batch"""
        _bind_kws(self._L)
        ss = [_f32(s).reshape(-1) for s in samples]
        B = len(ss)
        ptrs = (fp * B)(*[_f(s) for s in ss])
        ns = np.array([s.size for s in ss], np.int64)
        if max_events is None:   # at most one event per frame
            max_events = max(1, self.encoder_out_frames(int(self.fbank_num_frames(int(ns.max()))) + 19))
        me = max(max_events, 1)
        k, st, en = (np.zeros((B, me), np.int32) for _ in range(3))
        sm, sc = (np.zeros((B, me), np.float32) for _ in range(2))
        n = np.zeros(B, np.int32)
        tp = C.c_int32(0)
        self._chk(self._L.k2hip_offline_spot_keywords_from_samples(self._h, keywords._h, ptrs, _l(ns), B, _i(k), _i(st), _i(en), _f(sm), _f(sc),
                                                                   _i(n), max_events, C.byref(tp)))
        return [_kws_events(k[b], st[b], en[b], sm[b], sc[b], int(n[b])) for b in range(B)]

    # ---- keyword spotting for CTC models (k2hip.h "Keyword spotting for CTC models ...")
    def ctc_spot_keywords(self, log_probs, keywords: "Keywords", n_frames=None):
        """fresh CTC keyword streams over host log_probs [B,T',V] in one chunk -> per stream the list of events
        dict(keyword, start, end, sum_logp, score)"""
        e = _f32(log_probs)
        streams = [CtcKeywordStream(self, keywords) for _ in range(e.shape[0])]
        try:
            CtcKeywordStream.search_chunk(streams, e, n_frames)
            return [s.events() for s in streams]
        finally:
            for s in streams:
                s.close()

    def ctc_spot_keywords_samples(self, samples: Sequence[np.ndarray], keywords: "Keywords", max_events: Optional[int] = None):
        """k2hip_offline_ctc_spot_keywords_from_samples: samples -> fbank -> pad -> encoder on the device, then ctc_spot_keywords() over
        all T' frames of the padded batch"""
        _bind_ctc_kws(self._L)
        ss = [_f32(s).reshape(-1) for s in samples]
        B = len(ss)
        ptrs = (fp * B)(*[_f(s) for s in ss])
        ns = np.array([s.size for s in ss], np.int64)
        if max_events is None:   # at most one event per frame
            max_events = max(1, self.encoder_out_frames(int(self.fbank_num_frames(int(ns.max()))) + 19))
        me = max(max_events, 1)
        k, st, en = (np.zeros((B, me), np.int32) for _ in range(3))
        sm, sc = (np.zeros((B, me), np.float32) for _ in range(2))
        n = np.zeros(B, np.int32)
        tp = C.c_int32(0)
        self._chk(self._L.k2hip_offline_ctc_spot_keywords_from_samples(self._h, keywords._h, ptrs, _l(ns), B, _i(k), _i(st), _i(en), _f(sm), _f(sc),
                                                                       _i(n), max_events, C.byref(tp)))
        return [_kws_events(k[b], st[b], en[b], sm[b], sc[b], int(n[b])) for b in range(B)]

    # ---- CTC forced alignment and full-sum scoring (k2hip.h "CTC forced alignment and full-sum scoring ...")
    @staticmethod
    def _ctc_align_result(lens, ts, en, yp, tot, best):
        return [dict(timestamps=ts[h, : lens[h]].tolist(), end_frames=en[h, : lens[h]].tolist(), token_log_probs=yp[h, : lens[h]].copy(),
                     total_logp=float(tot[h]), best_logp=float(best[h])) for h in range(len(lens))]

    def _ctc_align_buffers(self, what, targets, R, stream_of, max_tokens):
        H = len(targets)
        if stream_of is None and H != R:
            raise ValueError(f"{what}: {H} targets for {R} rows and no stream_of")
        so = None if stream_of is None else np.ascontiguousarray(stream_of, dtype=np.int32).reshape(-1)
        if so is not None and so.size != H:
            raise ValueError(f"{what}: stream_of has {so.size} entries for {H} targets")
        ids, lens = self._align_targets(targets)
        mt = max(1, int(lens.max()) if H else 1) if max_tokens is None else max_tokens
        shape = (max(H, 1), max(mt, 1))
        return H, so, ids, lens, mt, np.zeros(shape, np.int32), np.zeros(shape, np.int32), np.zeros(shape, np.float32), \
            np.zeros(max(H, 1), np.float32), np.zeros(max(H, 1), np.float32)

    def ctc_align(self, log_probs, targets, n_frames=None, stream_of=None, max_tokens: Optional[int] = None):
        """k2hip_ctc_align over host log_probs [R,T',V] (what the encoder entries of a CTC model return): the forced alignment of every
        target (token ids in [1, V)) and its full-sum score -> a list of dict(timestamps, end_frames, token_log_probs, total_logp,
        best_logp).  n_frames [R]: the frames of each row that count (default: all T'); stream_of [H]: the row each target is scored
        against (default: target h against row h)."""
        x = _f32(log_probs)
        R, Tp, _ = x.shape
        H, so, ids, lens, mt, ts, en, yp, tot, best = self._ctc_align_buffers("ctc_align", targets, R, stream_of, max_tokens)
        nf = None if n_frames is None else np.ascontiguousarray(n_frames, dtype=np.int32)
        self._L.k2hip_ctc_align.argtypes = [C.c_void_p, fp, C.c_int32, C.c_int32, ip, C.c_int32, ip, lp, ip, ip, ip, fp, fp, fp, C.c_int32]
        self._chk(self._L.k2hip_ctc_align(self._h, _f(x), R, Tp, None if nf is None else _i(nf), H, None if so is None else _i(so), _l(ids),
                                          _i(lens), _i(ts), _i(en), _f(yp), _f(tot), _f(best), mt))
        return self._ctc_align_result(lens, ts, en, yp, tot, best)

    def ctc_align_samples(self, samples: Sequence[np.ndarray], targets, stream_of=None, max_tokens: Optional[int] = None):
        """k2hip_offline_ctc_align_from_samples: samples -> fbank -> pad -> encoder on the device, then ctc_align() over all T' frames of
        the padded batch (the frames the CTC search decodes)"""
        ss = [_f32(s).reshape(-1) for s in samples]
        B = len(ss)
        H, so, ids, lens, mt, ts, en, yp, tot, best = self._ctc_align_buffers("ctc_align_samples", targets, B, stream_of, max_tokens)
        ptrs = (fp * B)(*[_f(s) for s in ss])
        ns = np.array([s.size for s in ss], np.int64)
        tp = C.c_int32(0)
        self._L.k2hip_offline_ctc_align_from_samples.argtypes = [C.c_void_p, C.POINTER(fp), lp, C.c_int32, C.c_int32, ip, lp, ip, ip, ip, fp, fp,
                                                                 fp, C.c_int32, ip]
        self._chk(self._L.k2hip_offline_ctc_align_from_samples(self._h, ptrs, _l(ns), B, H, None if so is None else _i(so), _l(ids), _i(lens),
                                                               _i(ts), _i(en), _f(yp), _f(tot), _f(best), mt, C.byref(tp)))
        return self._ctc_align_result(lens, ts, en, yp, tot, best)

    # ---- device-resident benchmark path
    def device_alloc(self, nbytes: int) -> int:
        p = C.c_void_p()
        self._chk(self._L.k2hip_device_alloc(self._h, nbytes, C.byref(p)))
        return p.value

    def device_free(self, ptr: int):
        self._chk(self._L.k2hip_device_free(self._h, C.c_void_p(ptr)))

    def device_upload(self, ptr: int, host: np.ndarray):
        h = np.ascontiguousarray(host)
        self._chk(self._L.k2hip_device_upload(self._h, C.c_void_p(ptr), h.ctypes.data_as(C.c_void_p), h.nbytes))

    def synchronize(self):
        self._chk(self._L.k2hip_synchronize(self._h))

    def offline_greedy_from_samples_dev(self, dev_ptr: int, n_each: int, B: int, max_tokens: Optional[int] = None):
        mt = max_tokens or max(1, self.encoder_out_frames(self.fbank_num_frames(n_each) + 19))
        tok = np.zeros((B, mt), np.int64)
        ts = np.zeros((B, mt), np.int32)
        n = np.zeros(B, np.int32)
        self._chk(self._L.k2hip_offline_greedy_from_samples_dev(self._h, C.c_void_p(dev_ptr), n_each, B, _l(tok), _i(ts), _i(n), mt))
        return self._unpack(tok, ts, n)


    # pipelined form: submit() returns a ticket, wait(ticket) returns that batch's results
    def offline_submit_samples_dev(self, dev_ptr: int, n_each: int, B: int, max_tokens: Optional[int] = None):
        mt = max_tokens or max(1, self.encoder_out_frames(self.fbank_num_frames(n_each) + 19))
        t = C.c_int32()
        self._chk(self._L.k2hip_offline_submit_samples_dev(self._h, C.c_void_p(dev_ptr), n_each, B, mt, C.byref(t)))
        return (t.value, B, mt)

    def host_alloc(self, shape, dtype=np.float32) -> np.ndarray:
        """page-locked host array (k2hip_host_alloc); release with host_free(array)"""
        nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        p = C.c_void_p()
        self._chk(self._L.k2hip_host_alloc(self._h, nbytes, C.byref(p)))
        buf = (C.c_char * nbytes).from_address(p.value)
        a = np.frombuffer(buf, dtype=dtype).reshape(shape)
        self._pinned = getattr(self, "_pinned", {})
        self._pinned[a.ctypes.data] = p.value
        return a

    def host_free(self, a: np.ndarray):
        p = getattr(self, "_pinned", {}).pop(a.ctypes.data, None)
        if p is not None:
            self._chk(self._L.k2hip_host_free(self._h, C.c_void_p(p)))

    def offline_submit_samples(self, samples: np.ndarray, max_tokens: Optional[int] = None):
        """pipelined submit of a [B, n] f32 batch that is still in host memory (H2D inside the pipeline)"""
        assert samples.dtype == np.float32 and samples.ndim == 2 and samples.flags.c_contiguous
        B, n_each = samples.shape
        mt = max_tokens or max(1, self.encoder_out_frames(self.fbank_num_frames(n_each) + 19))
        t = C.c_int32()
        self._chk(self._L.k2hip_offline_submit_samples(self._h, _f(samples), n_each, B, mt, C.byref(t)))
        return (t.value, B, mt)

    def offline_wait(self, ticket):
        t, B, mt = ticket
        tok = np.zeros((B, mt), np.int64)
        ts = np.zeros((B, mt), np.int32)
        n = np.zeros(B, np.int32)
        self._chk(self._L.k2hip_offline_wait(self._h, t, _l(tok), _i(ts), _i(n)))
        return self._unpack(tok, ts, n)


def _alternatives(model, L, prefix, h):
    """a stream's alternatives in pick order: [dict(tokens, timestamps, token_log_probs, score)] (entry 0 = the best result)"""
    num, get = getattr(L, prefix + "_num_alternatives"), getattr(L, prefix + "_get_alternative")
    num.argtypes = [C.c_void_p]
    get.argtypes = [C.c_void_p, C.c_int32, lp, ip, fp, C.c_int32, ip, fp]
    count = num(h)
    if count < 0:
        model._chk(count)
    out = []
    for i in range(count):
        n, sc = C.c_int32(0), C.c_float(0)
        cap = 64
        while True:
            tok, ts, yp = np.zeros(cap, np.int64), np.zeros(cap, np.int32), np.zeros(cap, np.float32)
            rc = get(h, i, _l(tok), _i(ts), _f(yp), cap, C.byref(n), C.byref(sc))
            if rc == -5 and cap < (1 << 24):   # K2HIP_ERR_CAPACITY: nothing was written
                cap *= 8
                continue
            model._chk(rc)
            break
        out.append(dict(tokens=tok[: n.value].tolist(), timestamps=ts[: n.value].tolist(), token_log_probs=yp[: n.value].copy(), score=float(sc.value)))
    return out


def _token_log_probs(model, L, prefix, h) -> np.ndarray:
    get = getattr(L, prefix + "_get_token_log_probs")
    get.argtypes = [C.c_void_p, fp, C.c_int32]
    cap = 64
    while True:
        out = np.zeros(cap, np.float32)
        rc = get(h, _f(out), cap)
        if rc == -5 and cap < (1 << 24):
            cap *= 8
            continue
        if rc < 0:
            model._chk(rc)
        return out[:rc].copy()


class OfflineStream:
    """OfflineStream.cs:7-99."""

    def __init__(self, model: Model):
        self._m = model
        self._L = model._L
        h = C.c_void_p()
        model._chk(self._L.k2hip_offline_stream_create(model.handle, C.byref(h)))
        self._h = h
        model._children.add(self)

    def close(self):
        if getattr(self, "_h", None):
            self._L.k2hip_offline_stream_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def add_samples(self, samples):  # AddSamples, OfflineStream.cs:43-57
        s = _f32(samples).reshape(-1)
        self._m._chk(self._L.k2hip_offline_stream_accept_samples(self._h, _f(s), s.size))

    def accept_waveform(self, sample_rate: int, samples):
        """samples at any rate: queued as they are, converted to the model's rate on the device when the frames are needed.  The
        stream's rate is fixed by its first samples."""
        s = _f32(samples).reshape(-1)
        self._m._chk(self._L.k2hip_offline_stream_accept_waveform(self._h, int(sample_rate), _f(s), s.size))

    @property
    def speech_length(self) -> int:  # OfflineInputEntity.SpeechLength
        return self._L.k2hip_offline_stream_speech_length(self._h)

    @property
    def speech(self) -> np.ndarray:  # OfflineInputEntity.Speech
        n = self.speech_length
        out = np.empty(n, np.float32)
        self._m._chk(self._L.k2hip_offline_stream_get_speech(self._h, _f(out), n))
        return out

    @property
    def tokens(self) -> List[int]:
        n = self._L.k2hip_offline_stream_num_tokens(self._h)
        out = np.zeros(max(n, 1), np.int64)
        self._m._chk(self._L.k2hip_offline_stream_get_tokens(self._h, _l(out), n))
        return out[:n].tolist()

    @property
    def timestamps(self) -> List[int]:
        n = self._L.k2hip_offline_stream_num_timestamps(self._h)
        out = np.zeros(max(n, 1), np.int32)
        self._m._chk(self._L.k2hip_offline_stream_get_timestamps(self._h, _i(out), n))
        return out[:n].tolist()

    def alternatives(self):
        """the N-best list of the last get_results made with Model.set_nbest(n > 1) (k2hip_offline_stream_*_alternative*)"""
        alts = _alternatives(self._m, self._L, "k2hip_offline_stream", self._h)
        _bind_rnn_lm(self._L)
        for i, a in enumerate(alts):   # the neural LM's total of the alternative (0.0 when nothing was rescored)
            v = C.c_float(0)
            self._m._chk(self._L.k2hip_offline_stream_get_alternative_lm_score(self._h, i, C.byref(v)))
            a["lm_score"] = float(v.value)
            a["lodr_score"] = self.alternative_lodr_score(i)
        return alts

    def alternative_lodr_score(self, i: int) -> float:
        """k2hip_offline_stream_get_alternative_lodr_score: the LODR total of alternative i that the rescoring added (0.0 when nothing was
        rescored, without a LODR LM, and while fusion is active)"""
        self._L.k2hip_offline_stream_get_alternative_lodr_score.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_float)]
        self._L.k2hip_offline_stream_get_alternative_lodr_score.restype = C.c_int32
        v = C.c_float(0)
        self._m._chk(self._L.k2hip_offline_stream_get_alternative_lodr_score(self._h, int(i), C.byref(v)))
        return float(v.value)

    def token_log_probs(self) -> np.ndarray:
        return _token_log_probs(self._m, self._L, "k2hip_offline_stream", self._h)


class OfflineRecognizer:
    """OfflineRecognizer.cs:12-91 on the HIP backend; decoding_method "greedy_search" (the reference's only method) or
    "modified_beam_search" (BASELINE.json configs[2]), or for a CTC model "ctc_prefix_beam_search" with beam / nbest (the streams then carry
    .alternatives()).  hotwords: a Hotwords graph, or a list of token-id phrases scored
    hotwords_score per matched token (sherpa's hotwords_file / hotwords_score); it biases modified_beam_search only.  ngram_lm: an
    NgramLm fused with weight ngram_lm_scale (sherpa's lm / lm_scale), modified_beam_search only.  ctc_prefix_biasing=True: a CTC model's
    ctc_prefix_beam_search uses both as well (Model.set_ctc_prefix_biasing); without it the recognizer behaves as before.  rnn_lm: an
    RnnLm that rescores the N-best lists of get_results with weight rnn_lm_scale (sherpa's RNN LM rescoring); needs nbest > 1, the
    alternatives then carry lm_score.  rnn_lm_fusion=True: the LM is fused into modified_beam_search instead (Model.set_rnn_lm_fusion):
    its term is added during the search, any nbest, and the lists are not rescored.  lodr_lm: an NgramLm (usually a bi-gram) subtracted
    with weight lodr_scale <= 0 wherever rnn_lm acts, in the rescoring or in the fused search (Model.set_lodr_lm)."""

    def __init__(self, weights_path: str, device: int = 0, decoding_method: str = "greedy_search", beam: int = 4, hotwords=None,
                 hotwords_score: float = 1.5, nbest: int = 1, ngram_lm: Optional["NgramLm"] = None, ngram_lm_scale: float = 0.3,
                 ctc_prefix_biasing: bool = False, rnn_lm: Optional["RnnLm"] = None, rnn_lm_scale: float = 0.5, rnn_lm_fusion: bool = False,
                 lodr_lm: Optional["NgramLm"] = None, lodr_scale: float = -0.1):
        self.model = Model(weights_path, device)
        self.model.set_decoding_method(decoding_method, beam)
        if nbest != 1:   # (streams then carry .alternatives() / .token_log_probs() after get_results)
            self.model.set_nbest(nbest)
        if hotwords is not None:
            if not isinstance(hotwords, Hotwords):
                hotwords = Hotwords(hotwords, hotwords_score, self.model.vocab_size)
            self.model.set_hotwords(hotwords)
        if ngram_lm is not None:
            self.model.set_ngram_lm(ngram_lm, ngram_lm_scale)
        if ctc_prefix_biasing:
            self.model.set_ctc_prefix_biasing(True)
        if rnn_lm is not None:
            self.model.set_rnn_lm(rnn_lm, rnn_lm_scale)
        if rnn_lm_fusion:
            self.model.set_rnn_lm_fusion(True)
        if lodr_lm is not None:
            self.model.set_lodr_lm(lodr_lm, lodr_scale)

    def create_offline_stream(self) -> OfflineStream:  # CreateOfflineStream :71-75
        return OfflineStream(self.model)

    def get_results(self, streams: Sequence[OfflineStream]):  # GetResults :85-91 (tokens, not text)
        B = len(streams)
        arr = (C.c_void_p * B)(*[s._h for s in streams])
        self.model._chk(self.model._L.k2hip_offline_recognizer_get_results(self.model.handle, arr, B))
        return [(s.tokens, s.timestamps) for s in streams]

    def get_result(self, stream: OfflineStream):  # GetResult :77-83
        self.model._chk(self.model._L.k2hip_offline_recognizer_get_result(self.model.handle, stream._h))
        return stream.tokens, stream.timestamps

    def decode_long(self, samples, sample_rate: Optional[int] = None, config: Optional[VadConfig] = None, max_batch: int = 32,
                    max_batch_frames: int = 32000, tokens: Optional[TokenTable] = None):
        """a long recording cut by the voice activity detector and decoded by segment (Model.recognize_long; no reference counterpart).
        Returns per segment dict(start_s, end_s, forced, batch, tokens, timestamps_s, text): times in seconds of the recording (a token's:
        its segment's start + its encoder frame), text from `tokens` (a TokenTable) or None."""
        m = self.model
        try:
            shift_s = int(m.meta("frame_shift_ms")) / 1000.0
        except K2HipError:
            shift_s = 0.01   # (the container's default)
        enc_s = shift_s * 4   # encoder frames per fbank frame: the offline models subsample by 4
        out = []
        for g in m.recognize_long(samples, sample_rate, config, max_batch, max_batch_frames):
            t0 = g["start"] * shift_s
            out.append(dict(start_s=t0, end_s=g["end"] * shift_s, forced=bool(g["forced"]), batch=g["batch"], tokens=g["tokens"],
                            timestamps_s=[t0 + t * enc_s for t in g["timestamps"]],
                            text=tokens.decode(g["tokens"]) if tokens is not None else None))
        return out

    def align(self, samples: Sequence[np.ndarray], targets):
        """forced alignment and full-sum score of targets[b] (token ids) on samples[b] (Model.align_samples, or Model.ctc_align_samples
        when the model is a CTC model; no reference counterpart)"""
        if self.model.meta("model_type") == "zipformer2ctc":
            return self.model.ctc_align_samples(samples, targets)
        return self.model.align_samples(samples, targets)

    def spot_keywords(self, samples: Sequence[np.ndarray], keywords: "Keywords"):
        """the events of `keywords` in samples[b] (Model.spot_keywords_samples, or Model.ctc_spot_keywords_samples for a zipformer2ctc
        model; no reference counterpart)"""
        if self.model.meta("model_type") == "zipformer2ctc":
            return self.model.ctc_spot_keywords_samples(samples, keywords)
        return self.model.spot_keywords_samples(samples, keywords)


# ============================== streaming: OnlineStream / OnlineRecognizer ===============================
_STATE_KINDS = {"key": 0, "nonlin": 1, "val1": 2, "val2": 3, "conv1": 4, "conv2": 5, "embed": 6, "lstm_h": 0, "lstm_c": 1, "conf_attn": 0, "conf_conv": 1,
                # Zipformer v1 streams (OnlineProjOfZipformer.cs:56-111)
                "avg": 1, "val": 2, "len": 7}


def _bind_online(L):
    if getattr(L, "_online_bound", False):
        return
    vp = C.c_void_p
    L.k2hip_online_stream_create.argtypes = [vp, C.POINTER(vp)]
    L.k2hip_online_stream_destroy.argtypes = [vp]
    L.k2hip_online_stream_reset.argtypes = [vp]
    L.k2hip_online_chunk_info.argtypes = [vp, ip, ip, ip]
    L.k2hip_online_stream_accept_samples.argtypes = [vp, fp, C.c_int64]
    L.k2hip_online_stream_accept_features.argtypes = [vp, fp, C.c_int64]
    L.k2hip_online_accept_samples_batch.argtypes = [vp, C.POINTER(vp), C.c_int32, C.POINTER(fp), lp]
    L.k2hip_online_accept_samples_matrix.argtypes = [vp, C.POINTER(vp), C.c_int32, vp, C.c_int64, C.c_int64]
    L.k2hip_online_stream_speech_length.restype = C.c_int64
    L.k2hip_online_stream_speech_length.argtypes = [vp]
    L.k2hip_online_stream_is_finished.argtypes = [vp, C.c_int32, ip]
    L.k2hip_online_step.argtypes = [vp, C.POINTER(vp), C.c_int32, ip, ip]
    L.k2hip_online_state_create.argtypes = [vp, C.POINTER(vp)]
    L.k2hip_online_state_destroy.argtypes = [vp]
    L.k2hip_online_state_processed_len.restype = C.c_int64
    L.k2hip_online_state_processed_len.argtypes = [vp]
    L.k2hip_online_encoder.argtypes = [vp, C.POINTER(vp), C.c_int32, fp, fp, C.c_int64]
    L.k2hip_online_stream_num_tokens.argtypes = [vp]
    L.k2hip_online_stream_num_timestamps.argtypes = [vp]
    L.k2hip_online_stream_get_tokens.argtypes = [vp, lp, C.c_int32]
    L.k2hip_online_stream_get_timestamps.argtypes = [vp, ip, C.c_int32]
    L.k2hip_online_stream_get_hyp.argtypes = [vp, lp]
    L.k2hip_online_stream_state.argtypes = [vp, C.c_int32, C.c_int32, fp, C.c_int64, lp]
    L.k2hip_online_stream_get_score.argtypes = [vp, fp]
    L.k2hip_beam_stream_create.argtypes = [vp, C.c_int32, C.POINTER(vp)]
    L.k2hip_beam_stream_destroy.argtypes = [vp]
    L.k2hip_beam_stream_reset.argtypes = [vp]
    L.k2hip_beam_search_chunk.argtypes = [vp, C.POINTER(vp), C.c_int32, fp, C.c_int32]
    L.k2hip_beam_stream_num_tokens.argtypes = [vp]
    L.k2hip_beam_stream_get_tokens.argtypes = [vp, lp, C.c_int32]
    L.k2hip_beam_stream_get_timestamps.argtypes = [vp, ip, C.c_int32]
    L.k2hip_beam_stream_get_score.argtypes = [vp, fp]
    L.k2hip_online_stream_set_hotwords.argtypes = [vp, vp]
    L.k2hip_beam_stream_set_hotwords.argtypes = [vp, vp]
    L.k2hip_ctc_prefix_stream_create.argtypes = [vp, C.c_int32, C.c_int32, C.POINTER(vp)]
    L.k2hip_ctc_prefix_stream_destroy.argtypes = [vp]
    L.k2hip_ctc_prefix_stream_reset.argtypes = [vp]
    L.k2hip_ctc_prefix_stream_num_frames.restype = C.c_int64
    L.k2hip_ctc_prefix_stream_num_frames.argtypes = [vp]
    L.k2hip_ctc_prefix_beam_search_chunk.argtypes = [vp, C.POINTER(vp), C.c_int32, fp, C.c_int32, ip]
    L.k2hip_ctc_prefix_stream_num_tokens.argtypes = [vp]
    L.k2hip_ctc_prefix_stream_get_tokens.argtypes = [vp, lp, C.c_int32]
    L.k2hip_ctc_prefix_stream_get_timestamps.argtypes = [vp, ip, C.c_int32]
    L.k2hip_ctc_prefix_stream_get_score.argtypes = [vp, fp]
    L.k2hip_online_stream_set_ctc_prefix_beam.argtypes = [vp, C.c_int32, C.c_int32]
    L._online_bound = True


class OnlineStream:
    """OnlineStream.cs:7-199 (feature FIFO + Hyp/Tokens/Timestamps; caches live in a GPU slot)."""

    def __init__(self, model: Model):
        self._m = model
        self._L = model._L
        _bind_online(self._L)
        h = C.c_void_p()
        model._chk(self._L.k2hip_online_stream_create(model.handle, C.byref(h)))
        self._h = h
        model._children.add(self)

    def reset(self):
        """back to a freshly created stream (same slot): for the next utterance on the same object"""
        self._m._chk(self._L.k2hip_online_stream_reset(self._h))

    def set_hotwords(self, hotwords: Optional["Hotwords"] = None):
        """k2hip_online_stream_set_hotwords: this stream's hotword graph under modified_beam_search; None detaches.  Only before the
        stream's first decoded chunk or after reset(); the stream keeps its own reference (hotwords.close() afterwards is fine)."""
        self._m._chk(self._L.k2hip_online_stream_set_hotwords(self._h, hotwords._h if hotwords is not None else None))

    def set_ctc_prefix_beam(self, beam: int, nbest: int = 1):
        """k2hip_online_stream_set_ctc_prefix_beam: a streaming CTC model's stream decodes with the prefix beam search carried across
        chunks (beam 1..8, nbest alternatives kept; 0 = off, the per-chunk collapse).  Only before the stream's first decoded chunk or
        after reset().  tokens then are [blank, blank] + the best prefix, timestamps absolute frames; score, alternatives() and
        token_log_probs() serve it."""
        self._m._chk(self._L.k2hip_online_stream_set_ctc_prefix_beam(self._h, beam, nbest))

    def set_ctc_prefix_biasing(self, on: bool = True):
        """k2hip_online_stream_set_ctc_prefix_biasing: the stream's carried prefix search reads the stream's own hotword graph
        (set_hotwords) and the model's n-gram LM; off by default.  Only before the stream's first decoded chunk or after reset().  The
        stream then reports the first entry in final order, score = (tot + ctx) - pending: re-read tokens after every step."""
        self._L.k2hip_online_stream_set_ctc_prefix_biasing.argtypes = [C.c_void_p, C.c_int32]
        self._m._chk(self._L.k2hip_online_stream_set_ctc_prefix_biasing(self._h, 1 if on else 0))

    def close(self):
        if getattr(self, "_h", None):
            self._L.k2hip_online_stream_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def add_samples(self, samples):  # AddSamples :57-79
        s = _f32(samples).reshape(-1)
        self._m._chk(self._L.k2hip_online_stream_accept_samples(self._h, _f(s), s.size))

    def accept_waveform(self, sample_rate: int, samples):
        """samples at any rate; the stream carries the resampler's state, so any chunking gives the same frames.  The stream's rate
        is fixed by its first samples until reset()."""
        s = _f32(samples).reshape(-1)
        self._m._chk(self._L.k2hip_online_stream_accept_waveform(self._h, int(sample_rate), _f(s), s.size))

    def add_features(self, feats):
        f = _f32(feats).reshape(-1, self._m.feature_dim)
        self._m._chk(self._L.k2hip_online_stream_accept_features(self._h, _f(f), f.shape[0]))

    @property
    def speech_length(self) -> int:
        return self._L.k2hip_online_stream_speech_length(self._h)

    @property
    def speech(self) -> np.ndarray:  # OnlineInputEntity.Speech: the buffered frames
        self._L.k2hip_online_stream_get_speech.argtypes = [C.c_void_p, fp, C.c_int64]
        n = self.speech_length
        out = np.empty(n, np.float32)
        self._m._chk(self._L.k2hip_online_stream_get_speech(self._h, _f(out), n))
        return out

    def is_finished(self, is_endpoint: bool = False) -> bool:  # IsFinished :124-161
        out = C.c_int32()
        self._m._chk(self._L.k2hip_online_stream_is_finished(self._h, int(is_endpoint), C.byref(out)))
        return bool(out.value)

    @property
    def tokens(self) -> List[int]:
        n = self._L.k2hip_online_stream_num_tokens(self._h)
        out = np.zeros(max(n, 1), np.int64)
        self._m._chk(self._L.k2hip_online_stream_get_tokens(self._h, _l(out), n))
        return out[:n].tolist()

    @property
    def timestamps(self) -> List[int]:
        n = self._L.k2hip_online_stream_num_timestamps(self._h)
        out = np.zeros(max(n, 1), np.int32)
        self._m._chk(self._L.k2hip_online_stream_get_timestamps(self._h, _i(out), n))
        return out[:n].tolist()

    @property
    def hyp(self) -> List[int]:
        out = np.zeros(2, np.int64)
        self._m._chk(self._L.k2hip_online_stream_get_hyp(self._h, _l(out)))
        return out.tolist()

    @property
    def score(self) -> float:
        """log-prob of the best hypothesis under modified_beam_search (k2hip_online_stream_get_score)"""
        out = C.c_float()
        self._m._chk(self._L.k2hip_online_stream_get_score(self._h, C.byref(out)))
        return out.value

    def alternatives(self):
        """the stream's current hypotheses under modified_beam_search, up to Model.set_nbest's n, in pick order"""
        return _alternatives(self._m, self._L, "k2hip_online_stream", self._h)

    def token_log_probs(self) -> np.ndarray:
        return _token_log_probs(self._m, self._L, "k2hip_online_stream", self._h)

    @property
    def processed_len(self) -> int:
        self._L.k2hip_online_stream_processed_len.restype = C.c_int64
        self._L.k2hip_online_stream_processed_len.argtypes = [C.c_void_p]
        return int(self._L.k2hip_online_stream_processed_len(self._h))

    def state(self, layer: int, kind: str) -> np.ndarray:
        n = C.c_int64()
        self._m._chk(self._L.k2hip_online_stream_state(self._h, layer, _STATE_KINDS[kind], None, 0, C.byref(n)))
        out = np.empty(n.value, np.float32)
        self._m._chk(self._L.k2hip_online_stream_state(self._h, layer, _STATE_KINDS[kind], _f(out), n.value, C.byref(n)))
        return out


class StreamBatch:
    """The handles of a fixed group of OnlineStreams as one ctypes array (what a native host keeps next to its stream objects)."""

    def __init__(self, streams):
        self.streams = list(streams)
        self.arr = (C.c_void_p * len(self.streams))(*[s._h.value for s in self.streams])

    def __len__(self):
        return len(self.streams)

    def __iter__(self):
        return iter(self.streams)

    def __getitem__(self, i):
        return self.streams[i]


class OnlineProj:
    """IOnlineProj (IOnlineProj.cs:65-71) on the HIP backend: the operator a host swaps in when it keeps the reference's own
    OnlineRecognizer loop.  States are handles (a slot of the device pool each); stack_states / unstack_states are the identity."""

    def __init__(self, weights_path: str, device: int = 0):
        self.model = Model(weights_path, device)
        _bind_online(self.model._L)
        a, b, c = C.c_int32(), C.c_int32(), C.c_int32()
        self.model._chk(self.model._L.k2hip_online_chunk_info(self.model.handle, C.byref(a), C.byref(b), C.byref(c)))
        self.chunk_length, self.shift_length, self.frames_per_chunk = a.value, b.value, c.value

    def get_encoder_init_states(self):  # GetEncoderInitStates, one stream
        h = C.c_void_p()
        self.model._chk(self.model._L.k2hip_online_state_create(self.model.handle, C.byref(h)))
        return h

    def free_states(self, state):
        self.model._chk(self.model._L.k2hip_online_state_destroy(state))

    def processed_len(self, state) -> int:
        return int(self.model._L.k2hip_online_state_processed_len(state))

    def encoder_proj(self, feats, states) -> np.ndarray:  # EncoderProj: the states advance in place
        B = len(states)
        x = _f32(feats).reshape(B, self.chunk_length, -1)
        # (a streaming CTC model's encoder entry ends in its CTC head: [B, T', V] log-probs)
        out = np.empty((B, self.frames_per_chunk, self.model.encoder_out_dim), np.float32)
        arr = (C.c_void_p * B)(*[s.value for s in states])
        self.model._chk(self.model._L.k2hip_online_encoder(self.model.handle, arr, B, _f(x), _f(out), out.size))
        return out

    def decoder_proj(self, y) -> np.ndarray:
        return self.model.decoder_proj(y)

    def joiner_proj(self, enc, dec) -> np.ndarray:
        return self.model.joiner_proj(enc, dec)


class BeamStream:
    """Operator level of the streaming modified beam search (k2hip_beam_stream_*): one stream's hypotheses, continued over
    encoder frames the caller computed (BeamStream.search_chunk).  tokens exclude the [blank, blank] prefix; timestamps are
    absolute frame indexes."""

    def __init__(self, model: Model, beam: int = 4):
        self._m = model
        self._L = model._L
        _bind_online(self._L)
        h = C.c_void_p()
        model._chk(self._L.k2hip_beam_stream_create(model.handle, beam, C.byref(h)))
        self._h = h
        model._children.add(self)
        self.beam = beam

    def close(self):
        if getattr(self, "_h", None):
            self._L.k2hip_beam_stream_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self):
        self._m._chk(self._L.k2hip_beam_stream_reset(self._h))

    def set_hotwords(self, hotwords: Optional["Hotwords"] = None):
        """k2hip_beam_stream_set_hotwords: this stream's hotword graph; None detaches.  Only in the start state (new or reset)."""
        self._m._chk(self._L.k2hip_beam_stream_set_hotwords(self._h, hotwords._h if hotwords is not None else None))

    @staticmethod
    def search_chunk(streams: Sequence["BeamStream"], enc_out):
        """continue every stream's search over enc_out [B, Tc, J] (k2hip_beam_search_chunk)"""
        m = streams[0]._m
        e = _f32(enc_out)
        B, Tc = len(streams), e.shape[1]
        assert e.ndim == 3 and e.shape[0] == B, e.shape
        arr = (C.c_void_p * B)(*[s._h.value for s in streams])
        m._chk(m._L.k2hip_beam_search_chunk(m.handle, arr, B, _f(e), Tc))

    @property
    def tokens(self) -> List[int]:
        n = self._L.k2hip_beam_stream_num_tokens(self._h)
        out = np.zeros(max(n, 1), np.int64)
        self._m._chk(self._L.k2hip_beam_stream_get_tokens(self._h, _l(out), n))
        return out[:n].tolist()

    @property
    def timestamps(self) -> List[int]:
        n = self._L.k2hip_beam_stream_num_tokens(self._h)
        out = np.zeros(max(n, 1), np.int32)
        self._m._chk(self._L.k2hip_beam_stream_get_timestamps(self._h, _i(out), n))
        return out[:n].tolist()

    @property
    def score(self) -> float:
        out = C.c_float()
        self._m._chk(self._L.k2hip_beam_stream_get_score(self._h, C.byref(out)))
        return out.value

    def alternatives(self):
        """the stream's current hypotheses, up to Model.set_nbest's n, in pick order (k2hip_beam_stream_*_alternative*)"""
        return _alternatives(self._m, self._L, "k2hip_beam_stream", self._h)

    def token_log_probs(self) -> np.ndarray:
        return _token_log_probs(self._m, self._L, "k2hip_beam_stream", self._h)


class CtcPrefixStream:
    """Operator level of the streaming CTC prefix beam search (k2hip_ctc_prefix_stream_*): one stream's live prefixes, continued over
    chunks of log-probs the caller computed (Model.ctc_prefix_beam_search_chunk).  After any chunking the prefixes are those of
    Model.ctc_prefix_beam_search over all frames so far, bit for bit; timestamps are absolute frame indexes."""

    def __init__(self, model: Model, beam: int = 4, nbest: int = 1):
        self._m = model
        self._L = model._L
        _bind_online(self._L)
        h = C.c_void_p()
        model._chk(self._L.k2hip_ctc_prefix_stream_create(model.handle, beam, nbest, C.byref(h)))
        self._h = h
        model._children.add(self)
        self.beam, self.nbest = beam, nbest

    def close(self):
        if getattr(self, "_h", None):
            self._L.k2hip_ctc_prefix_stream_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self):
        self._m._chk(self._L.k2hip_ctc_prefix_stream_reset(self._h))

    def set_hotwords(self, hotwords: Optional["Hotwords"] = None):
        """k2hip_ctc_prefix_stream_set_hotwords: this stream's hotword graph, read only with set_biasing(True); None detaches.  Only in
        the start state (new or reset); a reset keeps it."""
        self._L.k2hip_ctc_prefix_stream_set_hotwords.argtypes = [C.c_void_p, C.c_void_p]
        self._m._chk(self._L.k2hip_ctc_prefix_stream_set_hotwords(self._h, hotwords._h if hotwords is not None else None))

    def set_biasing(self, on: bool = True):
        """k2hip_ctc_prefix_stream_set_biasing: the per-stream switch (off by default): the carried search reads this stream's graph and
        the model's n-gram LM.  Only in the start state (new or reset); a reset keeps it."""
        self._L.k2hip_ctc_prefix_stream_set_biasing.argtypes = [C.c_void_p, C.c_int32]
        self._m._chk(self._L.k2hip_ctc_prefix_stream_set_biasing(self._h, 1 if on else 0))

    @property
    def num_frames(self) -> int:
        return int(self._L.k2hip_ctc_prefix_stream_num_frames(self._h))

    @property
    def tokens(self) -> List[int]:
        n = self._L.k2hip_ctc_prefix_stream_num_tokens(self._h)
        out = np.zeros(max(n, 1), np.int64)
        self._m._chk(self._L.k2hip_ctc_prefix_stream_get_tokens(self._h, _l(out), n))
        return out[:n].tolist()

    @property
    def timestamps(self) -> List[int]:
        n = self._L.k2hip_ctc_prefix_stream_num_tokens(self._h)
        out = np.zeros(max(n, 1), np.int32)
        self._m._chk(self._L.k2hip_ctc_prefix_stream_get_timestamps(self._h, _i(out), n))
        return out[:n].tolist()

    @property
    def score(self) -> float:
        out = C.c_float()
        self._m._chk(self._L.k2hip_ctc_prefix_stream_get_score(self._h, C.byref(out)))
        return out.value

    def alternatives(self):
        """the first min(nbest, live) prefixes in rank order: [dict(tokens, timestamps, token_log_probs, score)]"""
        return _alternatives(self._m, self._L, "k2hip_ctc_prefix_stream", self._h)

    def token_log_probs(self) -> np.ndarray:
        return _token_log_probs(self._m, self._L, "k2hip_ctc_prefix_stream", self._h)


class OnlineRecognizer:
    """OnlineRecognizer.cs:11-84 on the HIP backend; decoding_method "greedy_search" (the reference's) or "modified_beam_search"
    (hypotheses carried from chunk to chunk: include/k2hip.h).  ngram_lm: an NgramLm fused with weight ngram_lm_scale
    under modified_beam_search (every hypothesis carries its LM state across the chunk boundary).  rnn_lm with rnn_lm_fusion=True:
    an RnnLm fused with weight rnn_lm_scale under modified_beam_search, its LSTM state carried from chunk to chunk
    (Model.set_rnn_lm_stream_fusion); without rnn_lm_fusion the LM is attached and the streaming search ignores it.  lodr_lm: an
    NgramLm subtracted with weight lodr_scale <= 0 beside the fused rnn_lm, its state carried as well (Model.set_lodr_lm); ignored
    without an active fusion.  nbest > 1: the streams keep that many alternatives."""

    def __init__(self, weights_path: str, device: int = 0, decoding_method: str = "greedy_search", beam: int = 4,
                 ngram_lm: Optional["NgramLm"] = None, ngram_lm_scale: float = 0.3, rnn_lm: Optional["RnnLm"] = None,
                 rnn_lm_scale: float = 0.5, rnn_lm_fusion: bool = False, nbest: int = 1, lodr_lm: Optional["NgramLm"] = None,
                 lodr_scale: float = -0.1):
        self.model = Model(weights_path, device)
        _bind_online(self.model._L)
        self.model.set_decoding_method(decoding_method, beam)
        if nbest != 1:
            self.model.set_nbest(nbest)
        if ngram_lm is not None:
            self.model.set_ngram_lm(ngram_lm, ngram_lm_scale)
        if rnn_lm is not None:
            self.model.set_rnn_lm(rnn_lm, rnn_lm_scale)
        if rnn_lm_fusion:
            self.model.set_rnn_lm_stream_fusion(True)
        if lodr_lm is not None:
            self.model.set_lodr_lm(lodr_lm, lodr_scale)
        a, b, c = C.c_int32(), C.c_int32(), C.c_int32()
        self.model._chk(self.model._L.k2hip_online_chunk_info(self.model.handle, C.byref(a), C.byref(b), C.byref(c)))
        self.chunk_length, self.shift_length, self.frames_per_chunk = a.value, b.value, c.value
        mt = self.model.meta("model_type")
        nl = self.model.meta("num_encoder_layers")
        self.num_layers = sum(int(x) for x in nl.split(",")) if nl else 0
        # names of the per-layer caches of this operator's GetEncoderInitStates, and the floats of embed_states (Zipformer2 only)
        self.state_kinds = {"zipformer2": ["key", "nonlin", "val1", "val2", "conv1", "conv2"], "zipformer2ctc": ["key", "nonlin", "val1", "val2", "conv1", "conv2"],
                            "zipformer": ["len", "avg", "key", "val", "val2", "conv1", "conv2"], "conformer": ["conf_attn", "conf_conv"],
                            "lstm": ["lstm_h", "lstm_c"]}.get(mt, [])
        self.embed_state_floats = 128 * 3 * 19 if mt in ("zipformer2", "zipformer2ctc") else 0

    def create_online_stream(self, hotwords=None, hotwords_score: float = 1.5, ctc_prefix_beam: int = 0, nbest: int = 1,
                             ctc_prefix_biasing: bool = False) -> OnlineStream:  # CreateOnlineStream :60-64
        """hotwords: a Hotwords graph, or a list of token-id phrases scored hotwords_score per matched token -- the stream's own list
        (sherpa-onnx's CreateStream(hotwords)); it biases modified_beam_search only.  ctc_prefix_beam > 0 (a streaming CTC model):
        the stream decodes with the carried prefix beam search, keeping nbest alternatives (OnlineStream.set_ctc_prefix_beam);
        ctc_prefix_biasing: that search reads the stream's hotwords and the model's n-gram LM (OnlineStream.set_ctc_prefix_biasing)."""
        s = OnlineStream(self.model)
        if ctc_prefix_beam:
            s.set_ctc_prefix_beam(ctc_prefix_beam, nbest)
        if ctc_prefix_biasing:
            s.set_ctc_prefix_biasing(True)
        if hotwords is not None:
            if isinstance(hotwords, Hotwords):
                s.set_hotwords(hotwords)
            else:
                hw = Hotwords(hotwords, hotwords_score, self.model.vocab_size)
                try:
                    s.set_hotwords(hw)
                finally:
                    hw.close()   # (the stream keeps its own reference to the uploaded tables)
        return s

    def add_samples_batch(self, streams: Sequence[OnlineStream], samples: Sequence[np.ndarray]):
        """B AddSamples calls in one (one fbank launch when all streams are at the same position)."""
        B = len(streams)
        arr = self._handles(streams)
        if isinstance(samples, np.ndarray) and samples.ndim == 2 and samples.dtype == np.float32 and samples.strides[1] == 4 and samples.strides[0] % 4 == 0:
            # one [B, n] matrix (rows contiguous, any row stride): one call, no per-stream pointers
            self.model._chk(self.model._L.k2hip_online_accept_samples_matrix(self.model.handle, arr, B, C.c_void_p(samples.ctypes.data),
                                                                             samples.strides[0] // 4, samples.shape[1]))
            return
        ss = [_f32(x).reshape(-1) for x in samples]
        ptrs = (fp * B)(*[_f(x) for x in ss])
        n = np.array([x.size for x in ss], np.int64)
        self.model._chk(self.model._L.k2hip_online_accept_samples_batch(self.model.handle, arr, B, ptrs, _l(n)))

    def accept_waveform_batch(self, streams: Sequence[OnlineStream], sample_rate: int, samples: Sequence[np.ndarray]):
        """B accept_waveform calls at one rate in one."""
        B = len(streams)
        arr = self._handles(streams)
        ss = [_f32(x).reshape(-1) for x in samples]
        ptrs = (fp * B)(*[_f(x) for x in ss])
        n = np.array([x.size for x in ss], np.int64)
        self.model._chk(self.model._L.k2hip_online_accept_waveform_batch(self.model.handle, arr, B, int(sample_rate), ptrs, _l(n)))

    def get_results(self, streams: Sequence[OnlineStream]):
        """GetResults :76-84 (tokens, not text).  Returns (decoded flags, new-token counts)."""
        B = len(streams)
        arr = self._handles(streams)
        dec = np.zeros(B, np.int32)
        n = np.zeros(B, np.int32)
        self.model._chk(self.model._L.k2hip_online_step(self.model.handle, arr, B, _i(dec), _i(n)))
        return dec.tolist(), n.tolist()

    def batch(self, streams: Sequence[OnlineStream]) -> "StreamBatch":
        """A fixed group of streams as the native array of handles a C# / C host would hold (IntPtr[]): pass it to
        add_samples_batch / get_results instead of the list and no per-call scan of the streams happens."""
        return StreamBatch(streams)

    def _handles(self, streams):
        """ctypes array of the streams' handles; rebuilt only when the list changes (a serving loop passes the same list every 50 ms)"""
        if isinstance(streams, StreamBatch):
            return streams.arr
        key = tuple(s._h.value for s in streams)
        if getattr(self, "_hkey", None) != key:
            self._hkey = key
            self._harr = (C.c_void_p * len(streams))(*key)
        return self._harr
