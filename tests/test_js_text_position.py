"""ElemIds of a Text resolved to positions through the JavaScript host (automerge_classic_amd/js/test_text_position.js): the sessions
of tests/golden/text/text_positions.json change by change through index.js; at every checkpoint positionsOfText answers for every
element ever inserted, served by the engine (am355_text_position: gpuPosition) except on the state with a `remove` record, where the
probe on the reference's backend answers (positionFallbacks) and equals the recorded values; then every session on the probe alone."""
import os
import subprocess

import pytest

from test_js_host import JS, NODE, ROOT, _emu_env

REF = "/root/reference"   # (the reference tree of the build container, as in tests/test_js_host.py: the probe fallback IS the reference)


def _check(out):
    assert out.returncode == 0 and "text positions through the JS host: ok" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
    print(out.stdout)


@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_text_positions_through_the_js_host_emulated():
    env = _emu_env(AM355_RESORDER_VERIFY="1")
    _check(subprocess.run([NODE, os.path.join(JS, "test_text_position.js")], capture_output=True, text=True, env=env, timeout=600))


@pytest.mark.skipif(NODE is None or not os.path.isdir(REF), reason="needs node and the reference tree (build container only)")
def test_the_probe_fallback_equals_the_fixture_emulated():
    """The same, then the state with a `remove` record and every session once more on the probe of the reference's backend."""
    env = _emu_env(AM355_RESORDER_VERIFY="1", NODE_PATH=os.path.join(ROOT, "oracle", "js_shims", "node_modules"), AUTOMERGE_BACKEND_PATH=os.path.join(REF, "backend"))
    out = subprocess.run([NODE, os.path.join(JS, "test_text_position.js")], capture_output=True, text=True, env=env, timeout=600)
    _check(out)
    assert "by the probe alone" in out.stdout


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_text_positions_through_the_js_host_on_gpu():
    if not os.path.exists(os.path.join(JS, "am355_napi.node")):
        import __graft_entry__ as g
        g.build_js_addon()
    env = dict(os.environ, AM355_RESORDER_VERIFY="1")
    _check(subprocess.run([NODE, os.path.join(JS, "test_text_position.js")], capture_output=True, text=True, env=env, timeout=600))
