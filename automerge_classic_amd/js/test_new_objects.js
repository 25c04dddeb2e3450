// Changes that make objects through the JS host: index.js switches am355_set_resident_new_objects on for every context it makes, so a
// peer that receives `doc.cards.push({...})`, `doc.meta = {...}`, `doc.log = new Text()` call by call has the new objects merged into the
// state its context holds. The `cards` session of tests/golden/resident/new_objects.json (tools/fixtures/make_new_object_sessions.js:
// made by the reference's frontend, patches by its backend):
//   * batch by batch through Backend.applyChanges of index.js: every patch and the whole patch at the end are the fixture's;
//   * with the reference tree (AUTOMERGE_REF=<tree>, AUTOMERGE_BACKEND_PATH=<tree>/backend, NODE_PATH with the reference's dependencies) also through the reference's
//     frontend over this backend (Automerge.setDefaultBackend): the document is what the reference's own backend gives.
// residentNewObjectCalls must show every make-call served in place and none declined; no call may be left to the JS fallback and no
// state may be hydrated.
//   node automerge_classic_amd/js/test_new_objects.js
'use strict'
const fs = require('fs')
const path = require('path')
const assert = require('assert')
const Backend = require(path.join(__dirname, 'index.js'))
const REF = process.env.AUTOMERGE_REF
const plain = x => JSON.parse(JSON.stringify(x))

const fx = JSON.parse(fs.readFileSync(path.join(__dirname, '..', '..', 'tests', 'golden', 'resident', 'new_objects.json'), 'utf8'))
const session = fx.sessions.find(s => s.name === 'cards')
const batches = session.batches.map(b => b.map(x => new Uint8Array(Buffer.from(x, 'base64'))))
const makeCalls = session.makes.filter(Boolean).length

let state = { state: { changes: [], queue: [] }, heads: [] }   // (an empty backend state, as the wrapper's init makes it)
batches.forEach((batch, i) => {
  const [next, got] = Backend.applyChanges(state, batch)
  state = next
  assert.deepStrictEqual(plain(got), JSON.parse(session.patches[i]), `call ${i}: the patch differs from the reference backend's`)
})
assert.deepStrictEqual(plain(Backend.getPatch(state)), JSON.parse(session.whole_patch), 'the document differs from the reference\'s')
let served = Backend._residentNewObjectCalls()
assert.deepStrictEqual(served, [makeCalls, 0], 'make-calls (served in place, declined): ' + JSON.stringify(served))

let viaFrontend = false
if (REF) {
  const Automerge = require(path.join(REF, 'src', 'automerge'))
  const RefBackend = require(path.join(REF, 'backend'))
  Automerge.setDefaultBackend(RefBackend)
  let want = Automerge.init()
  for (const batch of batches) want = Automerge.applyChanges(want, batch)[0]
  Automerge.setDefaultBackend(Backend)
  let doc = Automerge.init()
  for (const batch of batches) doc = Automerge.applyChanges(doc, batch)[0]
  assert.deepStrictEqual(plain(doc), plain(want), 'the document the frontend builds over this backend differs from the one over the reference backend')
  assert.strictEqual(doc.cards.length, want.cards.length)
  served = Backend._residentNewObjectCalls()
  assert.deepStrictEqual(served, [2 * makeCalls, 0], 'make-calls over both peers (served in place, declined): ' + JSON.stringify(served))
  viaFrontend = true
}
const c = Backend._counters
assert.strictEqual(c.fallbackToJs, 0, 'a call was served by the JS fallback: ' + JSON.stringify(c))
assert.strictEqual(c.hydrations, 0, 'a state was hydrated: ' + JSON.stringify(c))
console.log(JSON.stringify({ calls: batches.length, makeCalls, servedInPlace: served[0], declined: served[1], viaFrontend, counters: c }))
console.log('new objects through the JS host: ok')
