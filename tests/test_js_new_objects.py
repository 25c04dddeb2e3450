"""Changes that make objects through the JavaScript host (automerge_classic_amd/js/test_new_objects.js): index.js switches
am355_set_resident_new_objects on for its contexts; the `cards` session of tests/golden/resident/new_objects.json must come out patch
for patch as the reference recorded it, every make-call served in place, nothing hydrated."""
import os
import subprocess

import pytest

from test_js_host import JS, NODE, ROOT, _emu_env


def _check(out):
    assert out.returncode == 0 and "new objects through the JS host: ok" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
    print(out.stdout)


@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_new_objects_through_the_js_host_emulated():
    env = _emu_env(AM355_RESORDER_VERIFY="1")
    if os.path.isdir("/root/reference"):   # (the build container: through the reference's frontend as well)
        env.update(NODE_PATH=os.path.join(ROOT, "oracle", "js_shims", "node_modules"), AUTOMERGE_REF="/root/reference",
                   AUTOMERGE_BACKEND_PATH="/root/reference/backend")
    _check(subprocess.run([NODE, os.path.join(JS, "test_new_objects.js")], capture_output=True, text=True, env=env, timeout=600))


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_new_objects_through_the_js_host_on_gpu():
    if not os.path.exists(os.path.join(JS, "am355_napi.node")):
        import __graft_entry__ as g
        g.build_js_addon()
    env = dict(os.environ, AM355_RESORDER_VERIFY="1")
    _check(subprocess.run([NODE, os.path.join(JS, "test_new_objects.js")], capture_output=True, text=True, env=env, timeout=600))
