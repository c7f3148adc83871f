"""No GPU: the kernel sources under percnn_amd/csrc/ carry no build-time experiment switches.

The policy: an A/B variant of a kernel lives in a scratch build or under tools/; when it loses, its number goes to
docs/NOTEBOOK.md and its code goes away.  What the preprocessor may still test in the library's sources are the six
instrumentation switches that tools, a test and the ABI use."""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "percnn_amd", "csrc")

INSTRUMENTATION = {"PI_TILE_TIMING", "PI_PERSIST_STAMPS", "PI_S1_TIMING", "PI_3D_TIMING", "PI_R3D_STAMPS",
                   "PERCNN_PI_LIB_RK4_TILE"}


def test_the_preprocessor_tests_the_instrumentation_switches_only():
    tested = set()
    for name in sorted(os.listdir(CSRC)):
        path = os.path.join(CSRC, name)
        if not os.path.isfile(path) or name.endswith((".o", ".so")):        # (a built tree: objects and libraries lie here too)
            continue
        with open(path, errors="replace") as f:
            text = f.read().replace("\\\n", " ")
        for cond in re.findall(r"^[ \t]*#[ \t]*(?:ifdef|ifndef|if|elif)\b([^\n]*)", text, flags=re.M):
            cond = re.sub(r"/\*.*?\*/|//.*", " ", cond)
            tested |= set(re.findall(r"[A-Za-z_]\w*", cond)) - {"defined"}
    assert tested == INSTRUMENTATION
