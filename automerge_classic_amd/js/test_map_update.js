// A map edited by key through the JS host: updateMap / getMapValues / locateMap of index.js, additions beside the reference's surface.
// The sessions of tests/golden/map/map_updates.json (tools/fixtures/make_map_updates.js: the reference's frontend + backend executed
// d.key = v / delete d.key / d.key.increment(n) and recorded the request, the binary change and the patch) go call by call through
// index.js: changes of other replicas through Backend.applyChanges, every recorded call through updateMap. The binary change and the
// patch are the recorded ones. Every updateMap call is served by the engine (am355_map_update: gpuMap grows by exactly the calls made,
// mapFallbacks and hydrations stay 0), the first change of an empty document included (a reset context is the empty document); the
// reads count in gpuMapLocate / mapLocateFallbacks, exactly as well.
// Then the same sessions with every call forced onto the JS path (the whole-document patch folded into preds, this module's own
// applyLocalChange): the same changes. RangeError and TypeError carry the reference's texts on both paths.
//   node automerge_classic_amd/js/test_map_update.js
'use strict'
const fs = require('fs')
const path = require('path')
const assert = require('assert')
const Backend = require(path.join(__dirname, 'index.js'))

const fx = JSON.parse(fs.readFileSync(path.join(__dirname, '..', '..', 'tests', 'golden', 'map', 'map_updates.json'), 'utf8'))
const c = Backend._counters
const bytes = x => new Uint8Array(Buffer.from(x, 'base64'))

function value([cls, v]) {
  if (cls === 'str' || cls === 'bool' || cls === 'null' || cls === 'int') return v
  if (cls === 'float64') return Number.isInteger(v) ? { value: v, datatype: 'float64' } : v
  if (cls === 'timestamp') return new Date(v)
  return { value: v, datatype: cls }
}
const opsOf = call => call.ops.map(op => (op[0] === 'set' ? { action: 'set', key: op[1], value: value(op[2]) } : op[0] === 'del' ? { action: 'del', key: op[1] } : { action: 'inc', key: op[1], value: op[2] }))

// the sessions call by call; returns [calls that made a change, with nothing to do, that threw, made onto an empty document]
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
      const run = () => Backend.updateMap(state, call.objectId, opsOf(call), { actor: call.actor, time: call.time })
      if (call.kind === 'throws') {
        const Class = call.error === 'RangeError' ? RangeError : TypeError
        assert.throws(run, e => e instanceof Class && e.message === call.message, where)
        n[2]++
      } else if (!call.request) {
        const r = run()
        assert.ok(r[0] === state && r[1] === null && r[2] === null, where)
        n[1]++
      } else {
        // what the keys hold before the call: the ids are the preds of the recorded ops (the frontend lists the greatest first)
        if (at) {
          const located = Backend.locateMap(state, call.objectId, call.request.ops.map(op => op.key))
          call.request.ops.forEach((op, k) => assert.deepStrictEqual(located[k].ids.slice().reverse(), op.pred, `${where}: ${op.key}`))
        }
        const [next, patch, change] = run()
        assert.ok(Buffer.from(change).equals(Buffer.from(call.change, 'base64')), `${where}: the binary change differs`)
        assert.deepStrictEqual(JSON.parse(JSON.stringify(patch)), JSON.parse(call.patch), `${where}: the patch differs`)
        assert.throws(run, /frozen|outdated/i, `${where}: the state handed in is used up`)
        state = next
        if (!at) n[3]++
        at++
        n[0]++
        if (!call.table) {
          const shown = JSON.parse(call.object), held = Backend.getMapValues(state, call.objectId, call.ops.map(op => op[1]))
          for (const key of Object.keys(held)) {
            const ids = Object.keys(held[key])
            assert.strictEqual(ids.length > 0, Object.prototype.hasOwnProperty.call(shown, key), `${where}: ${key}`)
            const top = ids.length && held[key][ids[ids.length - 1]]
            if (top && !top.objectId && top.datatype !== 'timestamp') assert.deepStrictEqual(top.value, shown[key], `${where}: ${key}`)
          }
        }
      }
    })
  }
  return n
}

const NAMES = ['root', 'nested', 'nested_inner', 'conflicts', 'counters', 'children', 'table', 'key_order', 'mixed_values', 'bounds']
const before = Object.assign({}, c)
const [made, nothing, threw, first] = play(NAMES)
assert.ok(made >= 60 && nothing >= 3 && threw >= 9 && first === 3, JSON.stringify([made, nothing, threw, first]))
assert.strictEqual(c.hydrations, 0, 'a state was hydrated: ' + JSON.stringify(c))
// updateMap counts in gpuMap / mapFallbacks, the reads (locateMap, getMapValues) in words of their own: every call that made a change
// or had nothing to do was served by am355_map_update, none fell back; a call that throws is decided on the engine and counts in neither
assert.strictEqual(c.gpuMap - before.gpuMap, made + nothing, 'updateMap calls served by the engine: ' + JSON.stringify(c))
assert.strictEqual(c.mapFallbacks - before.mapFallbacks, 0, 'an updateMap call took the JS path: ' + JSON.stringify(c))
assert.strictEqual(c.localFallbacks - before.localFallbacks, 0, JSON.stringify(c))
// the reads: one locateMap in front of every recorded change but the first of a document, one getMapValues behind every one but a table's
const tableCalls = fx.sessions.find(s => s.name === 'table').calls.filter(call => call.kind === 'update' && call.request).length
assert.strictEqual(c.gpuMapLocate - before.gpuMapLocate, (made - first) + (made - tableCalls), 'reads served by the engine: ' + JSON.stringify(c))
assert.strictEqual(c.mapLocateFallbacks - before.mapLocateFallbacks, 0, 'a read took the JS path: ' + JSON.stringify(c))

// the same sessions with every call on the JS path: the same changes, the same errors, and every call counted there
Backend._setSpliceOnEngine(false)
const mid = Object.assign({}, c)
const again = play(NAMES)
Backend._setSpliceOnEngine(true)
assert.deepStrictEqual(again, [made, nothing, threw, first])
assert.strictEqual(c.gpuMap, mid.gpuMap, 'an updateMap call was served by the engine with the switch off')
assert.strictEqual(c.gpuMapLocate, mid.gpuMapLocate, 'a read was served by the engine with the switch off')
assert.strictEqual(c.mapFallbacks - mid.mapFallbacks, made + nothing + threw, JSON.stringify(c))
assert.strictEqual(c.mapLocateFallbacks - mid.mapLocateFallbacks, (made - first) + (made - tableCalls), JSON.stringify(c))

// arguments that are none
const empty = { state: { changes: [], queue: [] }, heads: [] }
assert.throws(() => Backend.updateMap(empty, '_root', [{ action: 'set', key: 'a', value: { a: 1 } }], { actor: 'aa' }), TypeError)
assert.throws(() => Backend.updateMap(empty, '_root', [{ action: 'move', key: 'a' }], { actor: 'aa' }), TypeError)
assert.throws(() => Backend.updateMap(empty, '_root', [{ action: 'set', key: 'a', value: 1 }, { action: 'del', key: 'a' }], { actor: 'aa' }), RangeError)
assert.throws(() => Backend.updateMap(empty, '_root', [{ action: 'set', key: 'a', value: 1 }], {}), TypeError)
assert.deepStrictEqual(Backend.getMapValues(empty, '_root', ['a']), { a: {} })
console.log(JSON.stringify({ callsThatMadeAChange: made, nothingToDo: nothing, threw, counters: c }))
console.log('map updates through the JS host: ok')
