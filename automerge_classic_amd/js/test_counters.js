// Counter increments through the JS host: index.js switches am355_set_resident_counters on for every context it makes (unless
// MI355X_COUNTERS=0), so a peer that receives `doc.votes.increment()` call by call has the counter's stored map record rewritten in place. The
// `plain` session of tests/golden/resident/counters.json (tools/fixtures/make_counter_sessions.js: made by the reference's frontend,
// patches by its backend) goes batch by batch through Backend.applyChanges of index.js: every patch and the whole patch at the end are
// the fixture's. residentCounterCalls must show every increment call served in place and none declined; no call may be left to the JS
// fallback and no state may be hydrated.
//   node automerge_classic_amd/js/test_counters.js
'use strict'
const fs = require('fs')
const path = require('path')
const assert = require('assert')
assert.notStrictEqual(process.env.MI355X_COUNTERS, '0', 'run without MI355X_COUNTERS=0')
const Backend = require(path.join(__dirname, 'index.js'))
const plain = x => JSON.parse(JSON.stringify(x))

const fx = JSON.parse(fs.readFileSync(path.join(__dirname, '..', '..', 'tests', 'golden', 'resident', 'counters.json'), 'utf8'))
const session = fx.sessions.find(s => s.name === 'plain')
const batches = session.batches.map(b => b.map(x => new Uint8Array(Buffer.from(x, 'base64'))))
const incCalls = session.kinds.filter(k => k === 'inc' || k === 'list+inc').length
assert.ok(incCalls >= 8 && incCalls === batches.length - 1)

let state = { state: { changes: [], queue: [] }, heads: [] }   // (an empty backend state, as the wrapper's init makes it)
batches.forEach((batch, i) => {
  const [next, got] = Backend.applyChanges(state, batch)
  state = next
  assert.deepStrictEqual(plain(got), JSON.parse(session.patches[i]), `call ${i}: the patch differs from the reference backend's`)
})
assert.deepStrictEqual(plain(Backend.getPatch(state)), JSON.parse(session.whole_patch), 'the document differs from the reference\'s')
const served = Backend._residentCounterCalls()
assert.deepStrictEqual(served, [incCalls, 0], 'increment calls (served in place, declined): ' + JSON.stringify(served))
const c = Backend._counters
assert.strictEqual(c.fallbackToJs, 0, 'a call was served by the JS fallback: ' + JSON.stringify(c))
assert.strictEqual(c.hydrations, 0, 'a state was hydrated: ' + JSON.stringify(c))
console.log(JSON.stringify({ calls: batches.length, incCalls, servedInPlace: served[0], declined: served[1], counters: c }))
console.log('counters through the JS host: ok')
