// A plain list edited by position through the JS host: spliceList / setListItem / locateList of index.js, additions beside the
// reference's surface. The sessions of tests/golden/list/list_splices.json (tools/fixtures/make_list_splices.js: the reference's frontend
// + backend executed list.deleteAt / list.insertAt / list[i] = v and recorded the request, the binary change and the patch) go call by
// call through index.js: changes of other replicas through Backend.applyChanges, every recorded call through spliceList / setListItem.
// The binary change and the patch are the recorded ones; every call is served by the engine (am355_list_splice / am355_list_set):
// gpuListSplice grows, hydrations stay 0, and listSpliceFallbacks counts only the one call the engine refuses (REFUSED: a list with an
// element whose first edit is an `update`, for which a frontend made fresh from the patch has no elemId -- a RangeError on both paths).
// Then the same sessions with every call forced onto the JS path (the whole-document patch folded into elemIds and preds, this module's
// own applyLocalChange): the same changes. RangeError and TypeError carry the reference's texts on both paths.
//   node automerge_classic_amd/js/test_list_splice.js
'use strict'
const fs = require('fs')
const path = require('path')
const assert = require('assert')
const Backend = require(path.join(__dirname, 'index.js'))

const fx = JSON.parse(fs.readFileSync(path.join(__dirname, '..', '..', 'tests', 'golden', 'list', 'list_splices.json'), 'utf8'))
const c = Backend._counters
const bytes = x => new Uint8Array(Buffer.from(x, 'base64'))
const REFUSED = new Set(['counters 19'])
const NO_ELEM = /first edit is an `update`/

// a [class, v] pair of the fixture as spliceList / setListItem take it
function value([cls, v]) {
  if (cls === 'str' || cls === 'bool' || cls === 'null' || cls === 'int') return v
  if (cls === 'float64') return Number.isInteger(v) ? { value: v, datatype: 'float64' } : v
  if (cls === 'timestamp') return new Date(v)
  return { value: v, datatype: cls }
}
// runs restated from the requests' own rule, for locateList: the deletion ops of a recorded request
const runsOfRequest = request => request.ops.filter(op => op.action === 'del').map(op => ({ elemId: op.elemId, preds: op.pred, count: op.multiOp || 1, counter: false }))

// the sessions call by call; returns [calls that made a change, calls with nothing to do, calls that threw, calls refused]
function play(names) {
  const n = [0, 0, 0, 0]
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
      const options = { actor: call.actor, time: call.time }
      const run = (call.call || call.kind) === 'splice' ? () => Backend.spliceList(state, call.objectId, call.start, call.deletions, call.values.map(value), options)
        : () => Backend.setListItem(state, call.objectId, call.index, value(call.value), options)
      if (call.kind === 'throws') {
        const Class = call.error === 'RangeError' ? RangeError : TypeError
        assert.throws(run, e => e instanceof Class && e.message === call.message, where)
        n[2]++
      } else if (REFUSED.has(`${name} ${i}`)) {
        assert.throws(run, e => e instanceof RangeError && NO_ELEM.test(e.message), where)
        at++   // the session goes on with the reference's change, loaded anew: the engine's incremental patch does not take it either
        state = Backend.loadChanges({ state: { changes: [], queue: [] }, heads: [] }, changes.slice(0, at))
        n[3]++
      } else if (!call.request) {
        const r = run()
        assert.ok(r[0] === state && r[1] === null && r[2] === null, where)
        n[1]++
      } else {
        if (call.kind === 'splice' && call.deletions > 0) {   // the deleted range located first: the runs are the request's deletion ops
          const located = Backend.locateList(state, call.objectId, call.start, call.deletions)
          assert.deepStrictEqual(located.runs, runsOfRequest(call.request), where)
        }
        const [next, patch, change] = run()
        assert.ok(Buffer.from(change).equals(Buffer.from(call.change, 'base64')), `${where}: the binary change differs`)
        assert.deepStrictEqual(JSON.parse(JSON.stringify(patch)), JSON.parse(call.patch), `${where}: the patch differs`)
        assert.throws(run, /frozen|outdated/i, `${where}: the state handed in is used up`)
        state = next
        at++
        if (`${name} ${i}` !== 'counters 17') assert.strictEqual(Backend.locateList(state, call.objectId, 0, 0).length, call.length, where)
        else assert.throws(() => Backend.locateList(state, call.objectId, 0, 0), NO_ELEM, where)   // (the element REFUSED is about is there from here on)
        n[0]++
      }
    })
    assert.deepStrictEqual(JSON.parse(JSON.stringify(Backend.getPatch(state))), JSON.parse(session.whole_patch), `${name}: the document differs from the reference's`)
  }
  return n
}

const NAMES = ['typed', 'mixed_values', 'two_actors', 'conflicts', 'holes', 'children', 'counters', 'past_end', 'bounds']
const [made, nothing, threw, refused] = play(NAMES)
assert.ok(made >= 70 && nothing >= 2 && threw >= 12 && refused === REFUSED.size, JSON.stringify([made, nothing, threw, refused]))
assert.strictEqual(c.gpuListSplice, made + nothing, 'list calls served by the engine: ' + JSON.stringify(c))
assert.strictEqual(c.listSpliceFallbacks, refused, 'a list call took the JS path: ' + JSON.stringify(c))
assert.strictEqual(c.hydrations, 0, 'a state was hydrated: ' + JSON.stringify(c))
assert.strictEqual(c.localFallbacks, 0, JSON.stringify(c))

// the same sessions with every call on the JS path: the same changes, the same errors
Backend._setSpliceOnEngine(false)
const again = play(NAMES)
Backend._setSpliceOnEngine(true)
assert.deepStrictEqual(again, [made, nothing, threw, refused])
assert.strictEqual(c.gpuListSplice, made + nothing)
assert.strictEqual(c.listSpliceFallbacks, refused + made + nothing + threw + refused, JSON.stringify(c))

// values that are no list values
const empty = { state: { changes: [], queue: [] }, heads: [] }
for (const bad of [{ a: 1 }, [1], undefined, () => 1, { value: 1, datatype: 'bytes' }]) {
  assert.throws(() => Backend.spliceList(empty, '1@aa', 0, 0, [bad], { actor: 'aa' }), TypeError)
  assert.throws(() => Backend.setListItem(empty, '1@aa', 0, bad, { actor: 'aa' }), TypeError)
}
console.log(JSON.stringify({ callsOnTheEngine: made, callsOnTheJsPath: again[0], nothingToDo: nothing, threw, refused, counters: c }))
console.log('list splices through the JS host: ok')
