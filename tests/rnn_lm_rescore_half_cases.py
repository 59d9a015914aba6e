"""The half twin and the constants of the half-precision rescoring tests (k2hip_set_rnn_lm_rescoring_precision).  HalfTwin is
rnn_lm_twin.restate32 -- the text of include/k2hip.h in numpy -- with W_hh and h_{t-1} rounded by astype(float16) in the recurrent product
ONLY, in float64 or float32 arithmetic.  E16R: the largest per-token difference between that twin in float32 and in float64 over LMs A, B,
C of rnn_lm_cases and its six hypothesis sets, with and without eos -- the reference's own error under this arithmetic, because a last-bit
difference in h can flip an f16 rounding of the next operand (the argument of rnn_lm_half_cases.py).  Measured on the CPU
(test_rnn_lm_rescore_half.py holds it to this constant); the device gets 8 E16R + 1e-6 per token and P times that per total."""
import numpy as np

from rnn_lm_cases import LMS   # noqa: F401

E16R = 3.1e-6   # measured 3.006e-06
SETS = ("fall", "drawn33")   # the operator's cases on the device; "fall": lengths {0, 1, 2, 31, 32, 33} over 70 hypotheses
RECOGNIZER_SEED = 1          # rnn_lm_cases.RECOGNIZER["transducer"]'s own draw meets the gap condition under the half twin


def token_bound():
    return 8 * E16R + 1e-6


def total_bound(positions):
    return max(int(positions), 1) * token_bound()


def key_bound(n_tokens, scale):
    """what the device's lm total can move a transducer alternative's key (score + scale lm) / (n + 2) by"""
    return scale * total_bound(n_tokens + 1) / (n_tokens + 2)


class HalfTwin:
    def __init__(self, sd, num_layers, dtype=np.float64, half=True, sos_id=1, eos_id=1):
        f = self.f = dtype
        self.L, self.sos, self.eos, self.H = num_layers, sos_id, eos_id, sd["rnn.weight_hh_l0"].shape[1]
        self.r = (lambda a: np.asarray(a).astype(np.float16).astype(f)) if half else (lambda a: np.asarray(a, f))
        self.emb, self.wo, self.bo = (np.asarray(sd[k], f) for k in ("input_embedding.weight", "output_linear.weight", "output_linear.bias"))
        self.wi = [np.asarray(sd[f"rnn.weight_ih_l{k}"], f) for k in range(num_layers)]
        self.wh = [self.r(sd[f"rnn.weight_hh_l{k}"]) for k in range(num_layers)]
        self.b = [np.asarray(sd[f"rnn.bias_ih_l{k}"], f) + np.asarray(sd[f"rnn.bias_hh_l{k}"], f) for k in range(num_layers)]

    def score(self, hyp, with_eos=True):
        """(total, token log-probs [positions]) of one hypothesis"""
        f, H = self.f, self.H
        sig = lambda v: f(1) / (f(1) + np.exp(-v, dtype=f))   # noqa: E731
        x, y = [self.sos] + [int(t) for t in hyp], [int(t) for t in hyp] + [self.eos]
        h, c = [np.zeros(H, f) for _ in range(self.L)], [np.zeros(H, f) for _ in range(self.L)]
        lps = np.zeros(len(hyp) + int(with_eos), f)
        for t in range(len(lps)):
            inp = self.emb[x[t]]
            for k in range(self.L):
                g = self.wi[k] @ inp + self.b[k]   # (GX: the unrounded input)
                if t:                              # (position 0 has no product)
                    g = g + self.wh[k] @ self.r(h[k])
                c[k] = sig(g[H: 2 * H]) * c[k] + sig(g[:H]) * np.tanh(g[2 * H: 3 * H], dtype=f)
                inp = h[k] = sig(g[3 * H:]) * np.tanh(c[k], dtype=f)
            z = self.wo @ inp + self.bo
            lps[t] = z[y[t]] - (z.max() + np.log(np.exp(z - z.max(), dtype=f).sum(dtype=f), dtype=f))
        return float(lps.sum(dtype=np.float64)), lps

    def score_all(self, hyps, with_eos=True):
        r = [self.score(h, with_eos) for h in hyps]
        return np.array([t for t, _ in r], np.float64), [lp for _, lp in r]
