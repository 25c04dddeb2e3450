"""Small local changes through the JavaScript host (automerge_classic_amd/js/test_local_small.js): the wrapper switches
am355_set_local_small on for every context (MI355X_LOCAL_SMALL=1 here; it is the default unless MI355X_LOCAL_SMALL=0), and the sessions of tests/golden/local/sessions.json go call by call through
Backend.load / applyChanges / applyLocalChange of index.js on the product library. Every returned binaryChange and patch is the recorded
one, addon.localSmallCalls over the contexts shows that the one workgroup built the changes, and localFallbacks counts the rejected
requests only. AM355_LOCAL_SMALL_VERIFY=1: every small build is repeated by the bulk path and compared. GPU only."""
import os
import subprocess

import pytest

from test_js_host import JS, NODE


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_small_local_changes_through_the_js_host_on_gpu():
    if not os.path.exists(os.path.join(JS, "am355_napi.node")):
        import __graft_entry__ as g
        g.build_js_addon()
    env = dict(os.environ, AM355_RESORDER_VERIFY="1", AM355_COUNTERS_VERIFY="1", AM355_LOCAL_SMALL_VERIFY="1", MI355X_LOCAL_SMALL="1")
    out = subprocess.run([NODE, os.path.join(JS, "test_local_small.js")], capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0 and "small local changes through the JS host: ok" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
    print(out.stdout)
