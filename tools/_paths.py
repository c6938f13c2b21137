"""Shared by the diagnostics in tools/: `import _paths` makes the package, the oracle and the test helpers of this checkout importable."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "hm-16.2_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), ROOT]
