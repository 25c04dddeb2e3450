// Key assignments through the JS host: with MI355X_MAP_MERGE=1 (set below) index.js switches am355_set_resident_map_merge on for the
// contexts it makes, so a peer that receives rounds of key assignments call by call has them merged into the map records its context holds.
//   * with the reference tree (AUTOMERGE_REF=<tree>, NODE_PATH with the reference's dependencies): two writers make rounds of
//     Automerge.change key assignments, overwrites and deletions with the reference's frontend and backend; every round's changes go
//     through Backend.applyChanges of index.js and of the reference backend: every patch and the final document are equal;
//   * without it (the GPU box): the reference-made changes of tests/golden/map_keys_small.json, change by change; the final patch
//     is the fixture's.
// Each session runs for TWO receiving peers, each in a context of its own (the module's first one and one acquireContext makes): both
// have the switch. residentMapMergeCalls must grow for both, nothing may decline, and no call may be left to the JS fallback.
//   node automerge_classic_amd/js/test_map_merge.js
'use strict'
const fs = require('fs')
const path = require('path')
const assert = require('assert')
process.env.MI355X_MAP_MERGE = '1'
const Backend = require(path.join(__dirname, 'index.js'))
const REF = process.env.AUTOMERGE_REF
const empty = () => ({ state: { changes: [], queue: [] }, heads: [] })

function rounds() {
  if (!REF) {
    const fx = JSON.parse(fs.readFileSync(path.join(__dirname, '..', '..', 'tests', 'golden', 'map_keys_small.json'), 'utf8'))
    const [c1, c2, c3] = fx.changes.map(x => new Uint8Array(Buffer.from(x, 'base64')))
    return { batches: [[c1], [c3], [c2]], patch: fx.patch, ref: null }
  }
  const Automerge = require(path.join(REF, 'src', 'automerge'))
  const RefBackend = require(path.join(REF, 'backend'))
  Automerge.setDefaultBackend(RefBackend)
  let a = Automerge.from({ title: 'first', nested: { x: 0 } }, 'aaaa')
  let b = Automerge.merge(Automerge.init('bbbb'), a)
  const batches = [Automerge.getAllChanges(a)]
  for (let r = 0; r < 12; r++) {
    a = Automerge.change(a, d => { for (let k = 0; k < 8; k++) d['k' + ((r * 5 + k) % 23)] = 'a' + r + '.' + k; d.nested['n' + (r % 4)] = r; if (r % 3 === 2) delete d['k' + (r % 23)] })
    b = Automerge.change(b, d => { for (let k = 0; k < 6; k++) d['k' + ((r * 3 + k) % 23)] = 'b' + r + '.' + k; d.nested.x = r; d['日本' + (r % 2)] = r })
    const ca = [Automerge.getLastLocalChange(a)], cb = [Automerge.getLastLocalChange(b)]
    batches.push(r % 2 ? ca.concat(cb) : ca)   // (the writers' changes of a round in one call, or one after the other)
    if (!(r % 2)) batches.push(cb)
    a = Automerge.merge(a, b)
    b = Automerge.merge(b, a)
  }
  return { batches, patch: null, ref: RefBackend }
}

const { batches, patch, ref } = rounds()
let calls = 0
for (let peer = 0; peer < 2; peer++) {
  let state = empty(), want = ref ? ref.init() : null
  for (const batch of batches) {
    const [next, got] = Backend.applyChanges(state, batch)
    state = next
    calls++
    if (ref) {
      const [w, wp] = ref.applyChanges(want, batch)
      want = w
      assert.deepStrictEqual(JSON.parse(JSON.stringify(got)), JSON.parse(JSON.stringify(wp)), `peer ${peer}, call ${calls}: the patch differs from the reference backend's`)
    }
  }
  const whole = JSON.parse(JSON.stringify(Backend.getPatch(state)))
  assert.deepStrictEqual(whole, ref ? JSON.parse(JSON.stringify(ref.getPatch(want))) : JSON.parse(patch), `peer ${peer}: the document differs from the reference's`)
}
const merged = Backend._residentMapMergeCalls(), c = Backend._counters
// (more than one peer's calls can account for: the first context serves a new author's first change by the full replay, the others do not)
assert(merged[0] >= batches.length, 'one of the two peers merged nothing in place: ' + JSON.stringify(merged))
assert(merged[0] > 0, 'no call merged its map rows in place: ' + JSON.stringify(merged))
assert.strictEqual(merged[1], 0, 'a call declined: ' + JSON.stringify(merged))
assert.strictEqual(c.fallbackToJs, 0, 'a call was served by the JS fallback: ' + JSON.stringify(c))
console.log(JSON.stringify({ calls, mergedInPlace: merged[0], declined: merged[1], withReferenceTree: !!REF, counters: c }))
console.log('map merge through the JS host: ok')
