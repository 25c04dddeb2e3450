// The string of a Text object through the JS host: getText / getTextInfo of index.js, additions beside the reference's surface. The
// `typed` and `conflicts` sessions of tests/golden/text/text_reads.json (tools/fixtures/make_text_reads.js: made by the reference's frontend,
// which also recorded the string and the length of the Text after every call) go batch by batch through Backend.applyChanges; after
// every call getText is the recorded string. Every read must be served by the engine (am355_object_text): gpuText grows, textFallbacks
// and hydrations stay 0. Then the same states read on the JS path (the whole-document patch folded by the rule): the same strings.
// An id that names no object, or no Text, throws a RangeError on both paths.
//   node automerge_classic_amd/js/test_text_read.js
'use strict'
const fs = require('fs')
const path = require('path')
const assert = require('assert')
const Backend = require(path.join(__dirname, 'index.js'))

const fx = JSON.parse(fs.readFileSync(path.join(__dirname, '..', '..', 'tests', 'golden', 'text', 'text_reads.json'), 'utf8'))
const c = Backend._counters
const noSuch = e => e instanceof RangeError && /^no such object: /.test(e.message)
const noText = e => e instanceof RangeError && e.message === 'not a Text object'

// the sessions call by call; returns the reads made
function play() {
  let reads = 0
  for (const name of ['typed', 'conflicts']) {
    const session = fx.sessions.find(s => s.name === name)
    assert.ok(session, name)
    const batches = session.batches.map(b => b.map(x => new Uint8Array(Buffer.from(x, 'base64'))))
    let state = { state: { changes: [], queue: [] }, heads: [] }   // (an empty backend state, as the wrapper's init makes it)
    batches.forEach((batch, i) => {
      state = Backend.applyChanges(state, batch)[0]
      for (const t of session.texts[i]) {
        assert.strictEqual(Backend.getText(state, t.objectId), t.string, `${name} call ${i}: getText of ${t.objectId}`)
        const info = Backend.getTextInfo(state, t.objectId)
        assert.strictEqual(info.text, t.string)
        assert.strictEqual(info.length, t.length, `${name} call ${i}: length of ${t.objectId}`)
        assert.ok(info.strings <= info.length)
        reads += 2
      }
    })
    const [ctr, actor] = session.texts[session.texts.length - 1][0].objectId.split('@')
    assert.throws(() => Backend.getText(state, `${Number(ctr) + 99999}@${actor}`), noSuch)
    assert.throws(() => Backend.getText(state, `${ctr}@${'0'.repeat(actor.length)}`), noSuch)
    assert.throws(() => Backend.getText(state, '_root'), noText)
    assert.deepStrictEqual(JSON.parse(JSON.stringify(Backend.getPatch(state))), JSON.parse(session.whole_patch), `${name}: the document differs from the reference's`)
  }
  return reads
}

const reads = play()
assert.strictEqual(c.gpuText, reads, 'reads served by the engine: ' + JSON.stringify(c))
assert.strictEqual(c.textFallbacks, 2, 'a read took the JS path (beside the two of _root, which is no object id): ' + JSON.stringify(c))
assert.strictEqual(c.hydrations, 0, 'a state was hydrated: ' + JSON.stringify(c))
assert.strictEqual(c.fallbackToJs, 0, 'a call was served by the JS fallback: ' + JSON.stringify(c))

// the same sessions with every read on the JS path: the same strings, the same errors
Backend._setTextOnEngine(false)
const folded = play()
Backend._setTextOnEngine(true)
assert.strictEqual(c.gpuText, reads)
assert.strictEqual(c.textFallbacks, 2 + folded + 6, JSON.stringify(c))
assert.strictEqual(c.hydrations, 0, 'a state was hydrated: ' + JSON.stringify(c))
console.log(JSON.stringify({ readsOnTheEngine: reads, readsOnTheJsPath: folded, counters: c }))
console.log('text reads through the JS host: ok')
