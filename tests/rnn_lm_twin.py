"""The neural LM of the rescoring feature without our code (helper of test_rnn_lm.py / test_rnn_lm_gpu.py).

`Twin` is torch's own nn.Embedding + nn.LSTM + nn.Linear + log_softmax in float64, loaded from the same state dict the container was
written from: it knows nothing of our gate order, our bias handling or our row layout.  `restate32` is the text of include/k2hip.h
("Neural LM rescoring") restated in float32 numpy: the yardstick whose error against the twin (E32 in rnn_lm_cases.py) sets the bound
the host reference and the device are held to."""
import numpy as np
import torch


class Twin:
    def __init__(self, sd, num_layers, sos_id=1, eos_id=1):
        V, E = sd["input_embedding.weight"].shape
        H = sd["rnn.weight_hh_l0"].shape[1]
        self.V, self.E, self.H, self.L, self.sos, self.eos = V, E, H, num_layers, sos_id, eos_id
        self.emb = torch.nn.Embedding(V, E).double()
        self.rnn = torch.nn.LSTM(E, H, num_layers, batch_first=True).double()
        self.out = torch.nn.Linear(H, V).double()
        with torch.no_grad():
            self.emb.weight.copy_(torch.from_numpy(np.asarray(sd["input_embedding.weight"], np.float64)))
            for k in range(num_layers):
                for p in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"):
                    getattr(self.rnn, f"{p}_l{k}").copy_(torch.from_numpy(np.asarray(sd[f"rnn.{p}_l{k}"], np.float64)))
            self.out.weight.copy_(torch.from_numpy(np.asarray(sd["output_linear.weight"], np.float64)))
            self.out.bias.copy_(torch.from_numpy(np.asarray(sd["output_linear.bias"], np.float64)))

    def score(self, hyp, with_eos=True):
        """(total, token log-probs [positions]) of one hypothesis in float64"""
        hyp = [int(t) for t in hyp]
        x = [self.sos] + hyp
        y = hyp + [self.eos]
        P = len(hyp) + (1 if with_eos else 0)
        if P == 0:
            return 0.0, np.zeros(0, np.float64)
        with torch.no_grad():
            h, _ = self.rnn(self.emb(torch.tensor([x[:P]], dtype=torch.long)))
            lp = torch.log_softmax(self.out(h[0]), dim=-1)
            lp = lp[torch.arange(P), torch.tensor(y[:P], dtype=torch.long)].numpy()
        return float(lp.sum()), lp

    def score_all(self, hyps, with_eos=True):
        r = [self.score(h, with_eos) for h in hyps]
        return np.array([t for t, _ in r], np.float64), [lp for _, lp in r]


def restate32(sd, num_layers, hyp, with_eos=True, sos_id=1, eos_id=1):
    """the header's formulas in float32 numpy: (total float32, token log-probs float32)"""
    f = np.float32
    emb = np.asarray(sd["input_embedding.weight"], f)
    H = sd["rnn.weight_hh_l0"].shape[1]
    wi = [np.asarray(sd[f"rnn.weight_ih_l{k}"], f) for k in range(num_layers)]
    wh = [np.asarray(sd[f"rnn.weight_hh_l{k}"], f) for k in range(num_layers)]
    b = [np.asarray(sd[f"rnn.bias_ih_l{k}"], f) + np.asarray(sd[f"rnn.bias_hh_l{k}"], f) for k in range(num_layers)]
    wo, bo = np.asarray(sd["output_linear.weight"], f), np.asarray(sd["output_linear.bias"], f)
    sig = lambda v: f(1) / (f(1) + np.exp(-v, dtype=f))   # noqa: E731
    hyp = [int(t) for t in hyp]
    x, y = [sos_id] + hyp, hyp + [eos_id]
    P = len(hyp) + (1 if with_eos else 0)
    h = [np.zeros(H, f) for _ in range(num_layers)]
    c = [np.zeros(H, f) for _ in range(num_layers)]
    lps, total = [], f(0)
    for t in range(P):
        inp = emb[x[t]]
        for k in range(num_layers):
            g = (wi[k] @ inp + b[k]) + wh[k] @ h[k]
            i, fg, gg, o = sig(g[:H]), sig(g[H: 2 * H]), np.tanh(g[2 * H: 3 * H], dtype=f), sig(g[3 * H:])
            c[k] = fg * c[k] + i * gg
            h[k] = o * np.tanh(c[k], dtype=f)
            inp = h[k]
        z = wo @ inp + bo
        m = z.max()
        lp = f(z[y[t]] - (m + np.log(np.exp(z - m, dtype=f).sum(dtype=f), dtype=f)))
        lps.append(lp)
        total = f(total + lp)
    return total, np.array(lps, f)


def plan_restated(lengths, with_eos=True, hidden_dim=32, gx_cap_floats=1 << 26):
    """csrc/rnn_lm_plan.h restated: dict(order, active, base, block)"""
    P = [int(n) + (1 if with_eos else 0) for n in lengths]
    order = sorted(range(len(P)), key=lambda i: (-P[i], i))
    T = max(P) if P else 0
    active = [sum(1 for p in P if p > t) for t in range(T)]
    base = [0]
    for a in active:
        base.append(base[-1] + a)
    cap_rows = max(gx_cap_floats // (4 * hidden_dim), 1)
    block = [0]
    for t in range(T):
        if t > block[-1] and base[t + 1] - base[block[-1]] > cap_rows:
            block.append(t)
    if T:
        block.append(T)
    return dict(order=order, active=active, base=base, block=block)


def rescored_order(scores, lengths, lm_totals, scale, ctc):
    """the re-ordering of an N-best list by the method's own quantity over score + scale * lm: (order, keys in float64)"""
    keys = [(s + scale * l) if ctc else (s + scale * l) / (n + 2) for s, n, l in zip(scores, lengths, lm_totals)]
    return sorted(range(len(keys)), key=lambda i: (-keys[i], i)), keys
