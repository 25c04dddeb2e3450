// A Text edited by position through the JS host: spliceText / locateText of index.js, additions beside the reference's surface. The
// sessions of tests/golden/text/text_splices.json (tools/fixtures/make_text_splices.js: the reference's frontend + backend executed
// text.deleteAt / text.insertAt and recorded the request, the binary change, the patch and the string) go call by call through
// index.js: changes of other replicas through Backend.applyChanges, every recorded splice through spliceText. The binary change, the
// patch and the string afterwards are the recorded ones; every splice is served by the engine (am355_text_splice): gpuSplice grows,
// spliceFallbacks and hydrations stay 0. Then the same sessions with every splice forced onto the JS path (the whole-document patch
// folded into elemIds and preds, this module's own applyLocalChange): the same changes. Out of bounds throws a RangeError with the
// reference's text and a deletion that reaches a Counter a TypeError, on both paths.
//   node automerge_classic_amd/js/test_text_splice.js
'use strict'
const fs = require('fs')
const path = require('path')
const assert = require('assert')
const Backend = require(path.join(__dirname, 'index.js'))

const fx = JSON.parse(fs.readFileSync(path.join(__dirname, '..', '..', 'tests', 'golden', 'text', 'text_splices.json'), 'utf8'))
const c = Backend._counters
const bytes = x => new Uint8Array(Buffer.from(x, 'base64'))
const COUNTER = 'Unsupported operation: deleting a counter from a list'

// runs of (elemId, pred) pairs restated from the requests' own rule, for locateText: the deletion ops of a recorded request
const runsOfRequest = request => request.ops.filter(op => op.action === 'del').map(op => ({ elemId: op.elemId, pred: op.pred[0], count: op.multiOp || 1, counter: false }))

// the sessions call by call; returns [splices that made a change, calls with nothing to do, calls that threw]
function play(names) {
  const n = [0, 0, 0]
  for (const name of names) {
    const session = fx.sessions.find(s => s.name === name)
    assert.ok(session, name)
    const changes = session.changes.map(bytes)
    let state = { state: { changes: [], queue: [] }, heads: [] }, at = 0   // (an empty backend state, as the wrapper's init makes it)
    session.calls.forEach((call, i) => {
      const where = `${name} call ${i}`
      assert.strictEqual(call.n_before, at, where)
      if (call.kind === 'apply') {
        state = Backend.applyChanges(state, changes.slice(at, at + call.n))[0]
        at += call.n
        return
      }
      const args = [call.objectId, call.start, call.deletions, call.values, { actor: call.actor, time: call.time }]
      if (call.kind === 'throws') {
        assert.throws(() => Backend.spliceText(state, ...args), e => e instanceof RangeError && e.message === call.message, where)
        n[2]++
      } else if (call.kind === 'counter') {
        assert.throws(() => Backend.spliceText(state, ...args), e => e instanceof TypeError && e.message === COUNTER, where)
        n[2]++
      } else if (!call.request) {
        const r = Backend.spliceText(state, ...args)
        assert.ok(r[0] === state && r[1] === null && r[2] === null, where)
        n[1]++
      } else {
        if (call.deletions > 0) {   // the deleted range located first: the runs are the request's deletion ops
          const located = Backend.locateText(state, call.objectId, call.start, call.deletions)
          assert.deepStrictEqual(located.runs, runsOfRequest(call.request), where)
        }
        // a string where the values are its code points, an array otherwise
        const joined = call.values.join('')
        if (call.values.length && [...joined].length === call.values.length && call.values.every((v, k) => v === [...joined][k])) args[3] = joined
        const [next, patch, change] = Backend.spliceText(state, ...args)
        assert.ok(Buffer.from(change).equals(Buffer.from(call.change, 'base64')), `${where}: the binary change differs`)
        assert.deepStrictEqual(JSON.parse(JSON.stringify(patch)), JSON.parse(call.patch), `${where}: the patch differs`)
        assert.throws(() => Backend.spliceText(state, ...args), /frozen|outdated/i, `${where}: the state handed in is used up`)
        state = next
        at++
        assert.strictEqual(Backend.getText(state, call.objectId), call.text, where)
        assert.strictEqual(Backend.locateText(state, call.objectId, 0, 0).length, call.length, where)
        n[0]++
      }
    })
    assert.deepStrictEqual(JSON.parse(JSON.stringify(Backend.getPatch(state))), JSON.parse(session.whole_patch), `${name}: the document differs from the reference's`)
  }
  return n
}

const NAMES = ['typed', 'conflicts', 'two_actors', 'holes', 'edges', 'counters']
const [made, nothing, threw] = play(NAMES)
assert.ok(made >= 50 && nothing >= 2 && threw >= 8, JSON.stringify([made, nothing, threw]))
assert.strictEqual(c.gpuSplice, made + nothing, 'splices served by the engine: ' + JSON.stringify(c))
assert.strictEqual(c.spliceFallbacks, 0, 'a splice took the JS path: ' + JSON.stringify(c))
assert.strictEqual(c.hydrations, 0, 'a state was hydrated: ' + JSON.stringify(c))
assert.strictEqual(c.fallbackToJs, 0, 'a call was served by the JS fallback: ' + JSON.stringify(c))
assert.strictEqual(c.localFallbacks, 0, JSON.stringify(c))

// the same sessions with every splice on the JS path: the same changes, the same errors
Backend._setSpliceOnEngine(false)
const [made2, nothing2, threw2] = play(NAMES)
Backend._setSpliceOnEngine(true)
assert.deepStrictEqual([made2, nothing2, threw2], [made, nothing, threw])
assert.strictEqual(c.gpuSplice, made + nothing)
assert.strictEqual(c.spliceFallbacks, made + nothing + threw, JSON.stringify(c))
console.log(JSON.stringify({ splicesOnTheEngine: made, splicesOnTheJsPath: made2, nothingToDo: nothing, threw, counters: c }))
console.log('text splices through the JS host: ok')
