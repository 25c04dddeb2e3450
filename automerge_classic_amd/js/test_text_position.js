// ElemIds of a Text resolved to positions through the JS host: positionsOfText of index.js, an addition beside the reference's surface.
// The sessions of tests/golden/text/text_positions.json (tools/fixtures/make_text_positions.js: every element ever inserted into a Text,
// with the position a probe on the reference's backend gives it) go change by change through Backend.applyChanges; at every checkpoint
// every recorded element is asked for. While the state is the engine's every call is served by it (am355_text_position): gpuPosition
// grows, positionFallbacks and hydrations stay 0 -- except at the checkpoint of `remove_record` (an increment of a deleted counter), the
// state the engine refuses: there the probe fallback answers, and its answers are the recorded ones. Then every session once more with
// every call forced onto the fallback: the probe on the reference's backend, equal to the fixture everywhere.
// The fallback IS the reference: those parts run where AUTOMERGE_BACKEND_PATH names its backend (and NODE_PATH its dependencies);
// without it the engine's part runs alone and stops in front of the change the engine leaves to the JS path.
//   node automerge_classic_amd/js/test_text_position.js
'use strict'
const fs = require('fs')
const path = require('path')
const assert = require('assert')
const Backend = require(path.join(__dirname, 'index.js'))

const fx = JSON.parse(fs.readFileSync(path.join(__dirname, '..', '..', 'tests', 'golden', 'text', 'text_positions.json'), 'utf8'))
const c = Backend._counters
const HAVE_REF = !!process.env.AUTOMERGE_BACKEND_PATH
const bytes = x => new Uint8Array(Buffer.from(x, 'base64'))
const wanted = cp => cp.queries.map(q => ({ status: q[1], position: q[2], counter: !!q[3] }))

// the sessions change by change; returns [checkpoints asked, of them on states the engine refuses]
function play(onEngine) {
  const n = [0, 0]
  for (const session of fx.sessions) {
    const changes = session.changes.map(bytes)
    let state = { state: { changes: [], queue: [] }, heads: [] }, at = 0   // (an empty backend state, as the wrapper's init makes it)
    for (const cp of session.checkpoints) {
      const where = `${session.name} after ${cp.n} changes`
      if (cp.refused && !HAVE_REF) break   // (the change that makes the `remove` record is the JS path's already)
      for (; at < cp.n; at++) state = Backend.applyChanges(state, [changes[at]])[0]
      const before = [c.gpuPosition, c.positionFallbacks]
      const got = Backend.positionsOfText(state, session.objectId, cp.queries.map(q => q[0]))
      assert.deepStrictEqual(got.positions, wanted(cp), where)
      assert.strictEqual(got.length, cp.length, where)
      const served = onEngine && !cp.refused
      assert.deepStrictEqual([c.gpuPosition - before[0], c.positionFallbacks - before[1]], served ? [1, 0] : [0, 1], `${where}: not served where it should be`)
      n[0]++
      if (cp.refused) n[1]++
    }
    // what is no Text, and what is no id
    assert.throws(() => Backend.positionsOfText(state, '_root', []), RangeError, session.name)
    assert.throws(() => Backend.positionsOfText(state, `999@${session.objectId.split('@')[1]}`, []), e => e instanceof RangeError && /no such object/.test(e.message), session.name)
    assert.throws(() => Backend.positionsOfText(state, session.objectId, ['_head']), TypeError, session.name)
    assert.deepStrictEqual(Backend.positionsOfText(state, session.objectId, []).positions, [], session.name)
  }
  return n
}

const hydrationsBefore = c.hydrations
const onEngine = play(true)
assert.ok(onEngine[0] >= 25 && onEngine[1] === (HAVE_REF ? 1 : 0), `checkpoints: ${onEngine}`)
const hydratedForEngine = c.hydrations - hydrationsBefore
if (!HAVE_REF) {
  assert.strictEqual(hydratedForEngine, 0)
  assert.strictEqual(c.positionFallbacks, fx.sessions.length)   // (`_root` has no id the engine could be asked with: the JS path says it is no Text, once per session)
  console.log(`text positions through the JS host: ok (${onEngine[0]} checkpoints on the engine; gpuPosition ${c.gpuPosition}, hydrations 0; the probe fallback needs the reference)`)
  process.exit(0)
}
Backend._setPositionOnEngine(false)
const gpuBefore = c.gpuPosition
const onJs = play(false)
Backend._setPositionOnEngine(true)
assert.deepStrictEqual(onJs, onEngine)
assert.strictEqual(c.gpuPosition, gpuBefore, 'a call forced onto the JS path was served by the engine')
// a loaded document that has not been changed takes the JS path; after its first change the engine serves it
{
  const session = fx.sessions.find(s => s.name === 'holes'), cp = session.checkpoints[session.checkpoints.length - 1]
  let state = Backend.applyChanges({ state: { changes: [], queue: [] }, heads: [] }, session.changes.map(bytes))[0]
  const loaded = Backend.load(Backend.save(state)), before = [c.gpuPosition, c.positionFallbacks]
  assert.deepStrictEqual(Backend.positionsOfText(loaded, session.objectId, cp.queries.map(q => q[0])).positions, wanted(cp), 'a loaded document')
  assert.deepStrictEqual([c.gpuPosition - before[0], c.positionFallbacks - before[1]], [0, 1], 'a loaded document')
}
console.log(`text positions through the JS host: ok (${onEngine[0]} checkpoints on the engine, ${onEngine[1]} of them refused and answered by the probe; ` +
  `${onJs[0]} by the probe alone; gpuPosition ${c.gpuPosition}, positionFallbacks ${c.positionFallbacks}, hydrations for the engine's answers ${hydratedForEngine})`)
