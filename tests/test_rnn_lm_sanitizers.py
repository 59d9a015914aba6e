"""The host side of the neural LM rescoring as its own program under AddressSanitizer / UBSan (tests/native/san_rnn_lm_driver.cpp,
`make san_rnn_lm`): the loader on truncated and mis-shaped files, the row plan on random length sets, the host reference, set / clear /
destroy in every order, and the re-ordering of the N-best lists with the new getter, all through the C ABI over the CPU stand-ins of the
engine.  Nothing is preloaded into Python."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_side_under_the_sanitizers(tiny_model_path, tmp_path):
    from k2transducerasr_amd.k2w import write_k2w
    from k2transducerasr_amd.synth import rnn_lm_state_dict, write_rnn_lm
    sd = rnn_lm_state_dict(37, 32, 32, 2, 9)
    good = str(tmp_path / "lm.k2w")
    write_rnn_lm(good, sd, 2)
    meta = {"model_type": "rnn_lm", "vocab_size": "37", "embedding_dim": "32", "hidden_dim": "32", "num_layers": "2", "sos_id": "1", "eos_id": "1",
            "tie_weights": "0"}
    bad = []

    def variant(name, meta_changes=None, drop=None, replace=None):
        t = {k: v for k, v in sd.items() if k != drop}
        t.update(replace or {})
        p = str(tmp_path / f"bad_{name}.k2w")
        write_k2w(p, dict(meta, **(meta_changes or {})), list(t.items()))
        bad.append(p)

    variant("missing", drop="rnn.weight_hh_l1")
    variant("short", replace={"rnn.weight_ih_l1": sd["rnn.weight_ih_l1"][:, :16].copy()})
    variant("tall", replace={"output_linear.bias": np.zeros(38, np.float32)})
    variant("rank", replace={"rnn.bias_hh_l0": sd["rnn.bias_hh_l0"].reshape(2, 64)})
    variant("i64", replace={"output_linear.weight": np.zeros((37, 32), np.int64)})
    nan = sd["input_embedding.weight"].copy()
    nan[36, 31] = np.nan
    variant("nan", replace={"input_embedding.weight": nan})
    variant("sos", meta_changes={"sos_id": "37"})
    variant("eos", meta_changes={"eos_id": "-2"})
    variant("layers", meta_changes={"num_layers": "3"})
    variant("vocab", meta_changes={"vocab_size": "99999999999"})
    variant("h48", meta_changes={"hidden_dim": "48"})
    variant("tied", meta_changes={"tie_weights": "1", "embedding_dim": "32", "hidden_dim": "32"}, drop="output_linear.bias")
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "k2transducerasr_amd", "csrc"), "-s", "san_rnn_lm"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(ROOT, "tests", "native", "k2hip_san_rnn_lm_driver"), tiny_model_path, good, str(tmp_path / "scratch.k2w")] + bad,
                       capture_output=True, text=True, env=env, timeout=600)
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0 and "san_rnn_lm_driver ok" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
