// Backend.applyLocalChange through the JS host: the sessions of tests/golden/local/sessions.json (tools/fixtures/
// make_local_change_sessions.js: requests made by the reference's frontend, binary changes and patches by its backend) go call by call
// through Backend.load / applyChanges / applyLocalChange of index.js. Every returned triple -- the state's heads, the patch, the binary
// change -- is the recorded one, the whole patch and Backend.save at the end too; every local call must be served by the engine
// (gpuApplyLocalChange), none left to the reference path, no state hydrated for it. The rejected requests must end on the reference
// path (the only hydrations): where the reference backend is installed they throw the recorded texts, elsewhere the attempt to load
// it is what fails.
//   node automerge_classic_amd/js/test_local_change.js
'use strict'
const fs = require('fs')
const path = require('path')
const crypto = require('crypto')
const assert = require('assert')
assert.notStrictEqual(process.env.MI355X_LOCAL_CHANGE, '0', 'run without MI355X_LOCAL_CHANGE=0')
const Backend = require(path.join(__dirname, 'index.js'))
const plain = x => JSON.parse(JSON.stringify(x))
const bytes = x => new Uint8Array(Buffer.from(x, 'base64'))

const fx = JSON.parse(fs.readFileSync(path.join(__dirname, '..', '..', 'tests', 'golden', 'local', 'sessions.json'), 'utf8'))
let haveReference = true
try { require(process.env.AUTOMERGE_BACKEND_PATH || 'automerge/backend') } catch (e) { haveReference = false }
let locals = 0, rejected = 0
for (const s of fx.sessions) {
  let state = { state: { changes: [], queue: [] }, heads: [] }   // (an empty backend state, as the wrapper's init makes it)
  let heads = []
  s.calls.forEach((call, i) => {
    const where = `${s.name} call ${i} (${call.kind})`
    if (call.kind === 'load') state = Backend.load(bytes(call.doc))
    else if (call.kind === 'remote') {
      const [next, patch] = Backend.applyChanges(state, call.batch.map(bytes))
      state = next
      assert.deepStrictEqual(plain(patch), JSON.parse(call.patch), where)
    } else if (call.kind === 'local') {
      const [next, patch, change] = Backend.applyLocalChange(state, plain(call.request))
      state = next
      locals++
      assert.deepStrictEqual(Buffer.from(change).toString('base64'), call.change, `${where}: the binary change`)
      assert.strictEqual(JSON.stringify(patch), call.patch, `${where}: the patch`)
      // the state's heads: the patch's deps and the new change's own hash (backend.js:88-90)
      assert.deepStrictEqual(next.heads, JSON.parse(call.patch).deps.concat([call.hash]).sort(), `${where}: heads`)
      assert.deepStrictEqual(Backend.getHeads(next), next.heads, `${where}: getHeads`)
    } else {
      const before = Backend._counters.localFallbacks
      let message = null
      try { Backend.applyLocalChange(state, plain(call.request)) } catch (e) { message = e.message }
      assert.notStrictEqual(message, null, `${where}: not rejected`)
      assert.strictEqual(Backend._counters.localFallbacks, before + 1, `${where}: the engine did not refuse it`)
      if (haveReference) assert.strictEqual(message, call.error, where)
      rejected++
      // (the reference froze the handle it was given, or was never loaded: the session goes on from the calls so far)
      state = { state: { changes: [], queue: [] }, heads: [] }
      for (const c of s.calls.slice(0, i)) {
        if (c.kind === 'local') state = Backend.applyChanges(state, [bytes(c.change)])[0]
        else if (c.kind === 'remote') state = Backend.applyChanges(state, c.batch.map(bytes))[0]
      }
    }
    heads = state.heads
  })
  assert.deepStrictEqual(plain(Backend.getPatch(state)), JSON.parse(s.whole_patch), `${s.name}: the document differs from the reference's`)
  assert.strictEqual(crypto.createHash('sha256').update(Backend.save(state)).digest('hex'), s.save_sha256, `${s.name}: Backend.save`)
  void heads
}
const c = Backend._counters
assert.ok(locals >= 30 && rejected === 3, JSON.stringify({ locals, rejected }))
assert.strictEqual(c.gpuApplyLocalChange, locals, 'local calls served by the engine: ' + JSON.stringify(c))
assert.strictEqual(c.localFallbacks, rejected, 'local calls left to the reference path: ' + JSON.stringify(c))
assert.strictEqual(c.fallbackToJs, 0, 'a call was served by the JS fallback: ' + JSON.stringify(c))
assert.strictEqual(c.hydrations, rejected, 'a served call hydrated a state (only the rejected requests reach the reference path): ' + JSON.stringify(c))
console.log(JSON.stringify({ sessions: fx.sessions.length, locals, rejected, haveReference, counters: c }))
console.log('local changes through the JS host: ok')
