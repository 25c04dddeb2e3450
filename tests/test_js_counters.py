"""Counter increments through the JavaScript host (automerge_classic_amd/js/test_counters.js): index.js switches
am355_set_resident_counters on for its contexts (MI355X_COUNTERS=1 here: also should the default change); the `plain` session of tests/golden/resident/counters.json must come out patch for
patch as the reference recorded it, every increment call served in place, none left to the JS fallback, nothing hydrated."""
import os
import subprocess

import pytest

from test_js_host import JS, NODE, _emu_env


def _check(out):
    assert out.returncode == 0 and "counters through the JS host: ok" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
    print(out.stdout)


@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_counters_through_the_js_host_emulated():
    env = _emu_env(AM355_RESORDER_VERIFY="1", AM355_COUNTERS_VERIFY="1", MI355X_COUNTERS="1")
    _check(subprocess.run([NODE, os.path.join(JS, "test_counters.js")], capture_output=True, text=True, env=env, timeout=600))


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_counters_through_the_js_host_on_gpu():
    if not os.path.exists(os.path.join(JS, "am355_napi.node")):
        import __graft_entry__ as g
        g.build_js_addon()
    env = dict(os.environ, AM355_RESORDER_VERIFY="1", AM355_COUNTERS_VERIFY="1", MI355X_COUNTERS="1")
    _check(subprocess.run([NODE, os.path.join(JS, "test_counters.js")], capture_output=True, text=True, env=env, timeout=600))
