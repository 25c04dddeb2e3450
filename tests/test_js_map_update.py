"""A map edited by key through the JavaScript host (automerge_classic_amd/js/test_map_update.js): the sessions of
tests/golden/map/map_updates.json call by call through index.js; every recorded d.key = v / delete d.key / d.key.increment(n) of the
reference's frontend is one updateMap whose binary change and patch are the recorded ones, served by the engine (am355_map_update; gpuMap)
wherever it holds the state; then the same sessions forced onto the JS path (mapFallbacks), and the RangeError / TypeError of both paths."""
import os
import subprocess

import pytest

from test_js_host import JS, NODE, _emu_env


def _check(out):
    assert out.returncode == 0 and "map updates through the JS host: ok" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
    print(out.stdout)


@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_map_updates_through_the_js_host_emulated():
    env = _emu_env(AM355_LOCAL_SMALL_VERIFY="1")
    _check(subprocess.run([NODE, os.path.join(JS, "test_map_update.js")], capture_output=True, text=True, env=env, timeout=600))


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_map_updates_through_the_js_host_on_gpu():
    if not os.path.exists(os.path.join(JS, "am355_napi.node")):
        import __graft_entry__ as g
        g.build_js_addon()
    env = dict(os.environ, AM355_LOCAL_SMALL_VERIFY="1")
    _check(subprocess.run([NODE, os.path.join(JS, "test_map_update.js")], capture_output=True, text=True, env=env, timeout=600))
