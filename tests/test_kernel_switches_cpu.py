"""CPU: the kernels' preprocessor conditionals test only the switches below - developer experiments are measured, recorded
under profiles/ and removed, not left in the source behind a macro of their own."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ALLOWED = {
    "MJMPC_STAMPS", "MJMPC_STAMPS_ABS", "MJMPC_STAMPS_MASK", "MJMPC_STAMPS_FENCE",     # tools/stamps.py
    "TREE_STATS", "TREE_STATS_FINE",                                                   # tools/tree_stats.py
    "MJMPC_NO_RESET",                                                                  # reset-cost A/B
    "MJMPC_ARM_XJ", "TREE_DENSE_TU", "TREE_CONE_TU",                                   # translation-unit selectors
}

DIRECTIVE = re.compile(r"^\s*#\s*(?:if|ifdef|ifndef|elif)\b(.*)$", re.M)


def _switches():
    found = {}
    for path in sorted(glob.glob(os.path.join(ROOT, "mjmpc_amd", "csrc", "*"))):
        if not path.endswith((".hip", ".h", ".inc")):
            continue
        for expr in DIRECTIVE.findall(open(path).read()):
            expr = expr.split("//")[0]
            for name in re.findall(r"\b[A-Za-z_]\w*\b", expr):
                if name != "defined":
                    found.setdefault(name, os.path.basename(path))
    return found


def test_kernel_switches_are_the_kept_ones():
    found = _switches()
    assert "MJMPC_STAMPS" in found and "TREE_DENSE_TU" in found        # (the scan sees the sources)
    stray = {name: where for name, where in found.items() if name not in ALLOWED}
    assert not stray, "preprocessor switches outside the kept list: %s" % stray
