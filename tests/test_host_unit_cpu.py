"""No GPU: the library's host runtime (percnn_amd/csrc/pi_host.hip) under the host's address and undefined-behaviour
sanitizers.  The unit holds no kernel, so it builds in seconds together with a stand-alone driver (tests/host_unit_main.hip:
the option parser on malformed strings, every option key by the field it lands in, the block decomposition of the direct
kernels over a grid of shapes) and the driver is run as a program of its own -- nothing is loaded into this interpreter.
Sanitizer runs belong on machines without a GPU: the test skips where one is present."""
import os
import subprocess

import pytest
import torch

from percnn_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.skipif(torch.cuda.is_available(), reason="host sanitizer run: CPU machines only")
def test_host_runtime_under_address_and_ub_sanitizers(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / "host_unit")
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17"] + san +
                          ["-o", exe, os.path.join(HERE, "host_unit_main.hip"), os.path.join(_lib.CSRC, "pi_host.hip")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    run = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr[-4000:]
    last = run.stdout.strip().splitlines()[-1]
    assert last.startswith("host unit ok: 58 option keys, "), run.stdout[-2000:]
    assert int(last.split()[-3]) > 100000                     # block maps computed
