"""The host side of the streaming neural LM shallow fusion as its own program under AddressSanitizer / UBSan
(tests/native/san_rnn_lm_stream_fusion_driver.cpp, `make san_rnn_lm_stream_fusion`): the state-block pool (csrc/rnn_lm_stream_pool.h)
over a heap allocator in random orders of create, first chunk, failed call (no flip), flip, reset, LM replaced, stream destroy and model
destroy before stream destroy, and the new API paths through the C ABI over the CPU stand-ins of the engine.  Nothing is preloaded
into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_driver(tiny_model_path, tmp_path):
    from k2transducerasr_amd.synth import write_synthetic_model, write_synthetic_rnn_lm
    sp = str(tmp_path / "streaming.k2w")
    write_synthetic_model(sp, "zipformer2-streaming-tiny-test")
    lms = []
    for i, (E, H, L) in enumerate([(32, 32, 2), (32, 96, 3)]):
        p = str(tmp_path / f"lm{i}.k2w")
        write_synthetic_rnn_lm(p, 37, E, H, L, 30 + i)
        lms.append(p)
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "k2transducerasr_amd", "csrc"), "-s", "san_rnn_lm_stream_fusion"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    return subprocess.run([os.path.join(ROOT, "tests", "native", "k2hip_san_rnn_lm_stream_fusion_driver"), tiny_model_path, sp] + lms, capture_output=True,
                          text=True, env=env, timeout=600)


def test_host_side_under_the_sanitizers(tiny_model_path, tmp_path):
    r = run_driver(tiny_model_path, tmp_path)
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0 and "san_rnn_lm_stream_fusion_driver ok" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
