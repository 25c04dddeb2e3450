"""Hash-graph queries through the JavaScript host (automerge_classic_amd/js/test_graph_queries.js): the histories of
tests/golden/graph/queries.json go through Backend.applyChanges of index.js on the product library, and every recorded
Backend.getChanges / getChangeByHash / getMissingDeps / getChangesAdded answer comes back byte for byte from the engine's index
lists: gpuChangesAdded counts the served pairs, no state is hydrated, nothing falls back to the reference path, and the result of
every getChangesAdded is applied onto the first state by the engine and ends at the recorded merged document. GPU only: the
emulated wrapper is covered by tests/test_js_host.py, which runs the reference's own suites and the sync campaign through it."""
import os
import subprocess

import pytest

from test_js_host import JS, NODE


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_graph_queries_through_the_js_host_on_gpu():
    if not os.path.exists(os.path.join(JS, "am355_napi.node")):
        import __graft_entry__ as g
        g.build_js_addon()
    out = subprocess.run([NODE, os.path.join(JS, "test_graph_queries.js")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "hash-graph queries through the JS host: ok" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
    print(out.stdout)
