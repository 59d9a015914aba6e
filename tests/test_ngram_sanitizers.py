"""CPU sanitizer builds (AddressSanitizer + UBSan) of the n-gram LM's host code: the text ARPA parser and the back-off automaton
(csrc/ngram_lm.cpp) over truncations and seeded mutations of a valid file and random walks, and the host layer with an LM set
(csrc/api.cpp) over the CPU stand-in of the engine -- a malformed file must come back as K2HIP_ERR_INVALID, never as a crash."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


@pytest.fixture(scope="module")
def drivers():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "k2transducerasr_amd", "csrc"), "-s", "san"])
    return os.path.join(NATIVE, "k2hip_san_ngram_driver"), os.path.join(NATIVE, "k2hip_san_ngram_api_driver")


def run(exe, *args):
    r = subprocess.run([exe, *args], capture_output=True, text=True, env=ENV, timeout=600)
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    return r.stdout.strip()


def test_arpa_parser_and_automaton_under_sanitizers(drivers):
    assert run(drivers[0]).startswith("san_ngram_driver: ok")


def test_host_layer_with_an_lm_set_under_sanitizers(drivers, tiny_model_path):
    assert run(drivers[1], tiny_model_path) == "san_ngram_api_driver: ok"
