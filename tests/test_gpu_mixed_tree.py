"""The coalescer's mixed takes together with the wake-up tree (SG_COALESCE_TREE, a process switch read once, so each case is a
process of its own: tests/mixed_tree_child.py).  A caller's waiter is thread-local and keeps the tree children of its last take;
plain and mixed takes alternate on the same threads, and a mixed take leaves two requests asleep for the next one — nobody may be
woken through a pointer of an earlier take.  The case without the tree runs the same takes, among them the requests that go back to
the queue because their key would be the 257th."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("tree", ["1", "0"])
def test_plain_and_mixed_takes_alternate_on_the_same_threads(tree):
    env = dict(os.environ, SG_COALESCE_TREE=tree)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "mixed_tree_child.py")], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out == {"tree": tree, "took": [[1, 0, 1], [2, 2, 258], [1, 0, 1]]}, out
