// Hash-graph queries through the JS host: the histories of tests/golden/graph/queries.json (tools/fixtures/make_graph_queries.js:
// made by the reference's frontend, answered by its backend) are delivered batch by batch through Backend.applyChanges of index.js,
// and every recorded Backend.getChanges / getChangeByHash / getMissingDeps / getChangesAdded answer must come back byte for byte --
// from the engine's index lists: no state is hydrated (the reference backend need not even be installed) and nothing falls back.
// After each getChangesAdded its result is applied onto the first state: served by the engine, ending at the recorded merged patch.
// Runs twice: the membership tests on the engine's host index and on the device (_setGraphProbeMin(1)).
//   node automerge_classic_amd/js/test_graph_queries.js
'use strict'
const fs = require('fs')
const path = require('path')
const assert = require('assert')
const Backend = require(path.join(__dirname, 'index.js'))
const plain = x => JSON.parse(JSON.stringify(x))
const bytes = x => new Uint8Array(Buffer.from(x, 'base64'))
const b64 = u8 => Buffer.from(u8.buffer, u8.byteOffset, u8.byteLength).toString('base64')
const empty = () => ({ state: { changes: [], queue: [] }, heads: [] })   // (an empty backend state, as the wrapper's init makes it)

const fx = JSON.parse(fs.readFileSync(path.join(__dirname, '..', '..', 'tests', 'golden', 'graph', 'queries.json'), 'utf8'))
const c = Backend._counters
let pairs = 0, answers = 0
for (const probeMin of [0xffffffff, 1]) {
  Backend._setGraphProbeMin(probeMin)
  const calls0 = Backend._graphQueryCalls()
  for (const h of fx.histories) {
    const changes = h.changes.map(bytes)
    const byHash = new Map(h.hashes.map((x, i) => [x, h.changes[i]]))
    const recorded = list => list.map(x => byHash.get(x))
    let state = empty(), at = 0
    for (const n of h.batches) { state = Backend.applyChanges(state, changes.slice(at, at + n))[0]; at += n }
    assert.deepStrictEqual(Backend.getHeads(state), h.heads, `${h.name}: heads`)
    assert.deepStrictEqual(Backend.getAllChanges(state).map(b64), recorded(h.applied), `${h.name}: getAllChanges`)
    for (const q of h.get_changes) {
      const where = `${h.name}: getChanges(${JSON.stringify(q.have).slice(0, 150)})`
      if (q.error !== undefined) assert.throws(() => Backend.getChanges(state, q.have), e => e instanceof RangeError && e.message === q.error, where)
      else assert.deepStrictEqual(Backend.getChanges(state, q.have).map(b64), recorded(q.result), where)
      answers++
    }
    for (const q of h.change_by_hash) {
      const got = Backend.getChangeByHash(state, q.hash)
      assert.strictEqual(got === undefined ? undefined : b64(got), q.found ? byHash.get(q.hash) : undefined, `${h.name}: getChangeByHash(${q.hash})`)
      answers++
    }
    for (const q of h.missing_deps) {
      assert.deepStrictEqual(Backend.getMissingDeps(state, q.heads), q.result, `${h.name}: getMissingDeps(${JSON.stringify(q.heads).slice(0, 150)})`)
      answers++
    }
    for (const p of h.changes_added) {
      const where = `${h.name}: getChangesAdded ${p.name}`
      const first = p.first.length ? Backend.applyChanges(empty(), p.first.map(i => changes[i]))[0] : empty()
      const second = p.second.length ? Backend.applyChanges(empty(), p.second.map(i => changes[i]))[0] : empty()
      if (!p.second.length) continue   // (an empty second state is the reference's own: nothing of the engine's to ask)
      const served = c.gpuChangesAdded, applies = c.gpuApplyChanges
      const added = Backend.getChangesAdded(first, second)
      assert.strictEqual(c.gpuChangesAdded, served + 1, `${where}: not served by the engine`)
      assert.deepStrictEqual(added.map(b64), recorded(p.result), where)
      pairs++
      // the other half of Automerge.merge: the result applied onto the first state, on the engine
      let merged = first
      if (added.length) {
        merged = Backend.applyChanges(first, added)[0]
        assert.strictEqual(c.gpuApplyChanges, applies + 1, `${where}: the merge was not applied by the engine`)
      }
      assert.deepStrictEqual(plain(Backend.getPatch(merged)), JSON.parse(p.merged_patch), `${where}: the merged document`)
    }
  }
  const calls1 = Backend._graphQueryCalls()
  if (probeMin === 1) assert.ok(calls1[0] > calls0[0], 'no membership test ran on the device: ' + JSON.stringify([calls0, calls1]))
  else assert.ok(calls1[1] > calls0[1] && calls1[0] === calls0[0], 'the host index was to answer: ' + JSON.stringify([calls0, calls1]))
}
assert.ok(pairs >= 30 && answers >= 300, JSON.stringify({ pairs, answers }))
assert.strictEqual(c.gpuChangesAdded, pairs, 'getChangesAdded pairs served by the engine: ' + JSON.stringify(c))
assert.strictEqual(c.hydrations, 0, 'a state was hydrated: ' + JSON.stringify(c))
assert.strictEqual(c.fallbackToJs, 0, 'a call was served by the JS fallback: ' + JSON.stringify(c))
console.log(JSON.stringify({ histories: fx.histories.length, pairs, answers, counters: c, graphQueryCalls: Backend._graphQueryCalls() }))
console.log('hash-graph queries through the JS host: ok')
