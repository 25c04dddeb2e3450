"""A plain list edited by position through the JavaScript host (automerge_classic_amd/js/test_list_splice.js): the sessions of
tests/golden/list/list_splices.json call by call through index.js; every recorded list.deleteAt / list.insertAt / list[i] = v of the
reference's frontend is one spliceList / setListItem whose binary change and patch are the recorded ones, served by the engine
(am355_list_splice / am355_list_set; gpuListSplice) -- but for the one call the engine refuses, which the JS path refuses too --; then the
same sessions forced onto the JS path (listSpliceFallbacks), and the RangeError / TypeError of both paths."""
import os
import subprocess

import pytest

from test_js_host import JS, NODE, _emu_env


def _check(out):
    assert out.returncode == 0 and "list splices through the JS host: ok" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
    print(out.stdout)


@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_list_splices_through_the_js_host_emulated():
    env = _emu_env(AM355_RESORDER_VERIFY="1", AM355_LOCAL_SMALL_VERIFY="1")
    _check(subprocess.run([NODE, os.path.join(JS, "test_list_splice.js")], capture_output=True, text=True, env=env, timeout=600))


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_list_splices_through_the_js_host_on_gpu():
    if not os.path.exists(os.path.join(JS, "am355_napi.node")):
        import __graft_entry__ as g
        g.build_js_addon()
    env = dict(os.environ, AM355_RESORDER_VERIFY="1", AM355_LOCAL_SMALL_VERIFY="1")
    _check(subprocess.run([NODE, os.path.join(JS, "test_list_splice.js")], capture_output=True, text=True, env=env, timeout=600))
