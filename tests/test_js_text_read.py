"""The string of a Text object through the JavaScript host (automerge_classic_amd/js/test_text_read.js): the `typed` and `conflicts`
sessions of tests/golden/text/text_reads.json call by call through index.js; after every applyChanges getText is the string the reference's
frontend recorded, every read served by the engine (am355_object_text), none by the JS path, nothing hydrated; then the same states
read on the JS path (the whole-document patch folded by the rule), and the RangeErrors of both paths."""
import os
import subprocess

import pytest

from test_js_host import JS, NODE, _emu_env


def _check(out):
    assert out.returncode == 0 and "text reads through the JS host: ok" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
    print(out.stdout)


@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_text_reads_through_the_js_host_emulated():
    env = _emu_env(AM355_RESORDER_VERIFY="1")
    _check(subprocess.run([NODE, os.path.join(JS, "test_text_read.js")], capture_output=True, text=True, env=env, timeout=600))


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_text_reads_through_the_js_host_on_gpu():
    if not os.path.exists(os.path.join(JS, "am355_napi.node")):
        import __graft_entry__ as g
        g.build_js_addon()
    env = dict(os.environ, AM355_RESORDER_VERIFY="1")
    _check(subprocess.run([NODE, os.path.join(JS, "test_text_read.js")], capture_output=True, text=True, env=env, timeout=600))
