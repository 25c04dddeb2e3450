"""Backend.applyLocalChange through the JavaScript host (automerge_classic_amd/js/test_local_change.js): the sessions of
tests/golden/local/sessions.json go call by call through Backend.load / applyChanges / applyLocalChange of index.js on the product
library. Every returned triple is the recorded one, every local call is served by the engine (gpuApplyLocalChange), none is left to
the reference path (localFallbacks counts the rejected requests only) and no served call hydrates a state. GPU only: the emulated
wrapper is covered by tests/test_js_host.py, which runs the reference's own suites through it."""
import os
import subprocess

import pytest

from test_js_host import JS, NODE


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_local_changes_through_the_js_host_on_gpu():
    if not os.path.exists(os.path.join(JS, "am355_napi.node")):
        import __graft_entry__ as g
        g.build_js_addon()
    env = dict(os.environ, AM355_RESORDER_VERIFY="1", AM355_COUNTERS_VERIFY="1")
    out = subprocess.run([NODE, os.path.join(JS, "test_local_change.js")], capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0 and "local changes through the JS host: ok" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
    print(out.stdout)
