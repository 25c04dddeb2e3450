// The string of the headline document's Text through the JS host: the engine's read (addon.objectText -> am355_object_text -> a JS
// string made from the pinned bytes) against the route of before -- the patch IR fetched and materialised (materialize.js, the
// bench_e2e.js path) and the patch folded into the string (index.js textFromPatch: what getText does on the JS path; the reference's
// frontend does more per element). Each timed behind a replay of its own, alternating.
//
//   python -c "from automerge_classic_amd import loggen; loggen.config('c4_text_single', 1.0, False).save('/tmp/c4.bin')"
//   node automerge_classic_amd/js/bench_text.js /tmp/c4.bin [reps]
//
// Log file layout (little endian): u32 n_changes, u64 n_ops, u64 offsets[n+1], arena.
'use strict'
const fs = require('fs')
const path = require('path')
const addon = require(path.join(__dirname, 'am355_napi.node'))
const { materialize } = require('./materialize.js')
const { _textFromPatch: textFromPatch } = require('./index.js')

const buf = fs.readFileSync(process.argv[2])
const reps = parseInt(process.argv[3] || '7')
const n = buf.readUInt32LE(0)
const nOps = Number(buf.readBigUInt64LE(4))
const offs = []
for (let i = 0; i <= n; i++) offs.push(Number(buf.readBigUInt64LE(12 + 8 * i)))
const base = 12 + 8 * (n + 1)
const changes = []
for (let i = 0; i < n; i++) changes.push(new Uint8Array(buf.buffer, buf.byteOffset + base + offs[i], offs[i + 1] - offs[i]))

const ctx = addon.create(parseInt(process.env.MI355X_DEVICE || '0'))
const ms = () => Number(process.hrtime.bigint()) / 1e6
addon.loadChanges(ctx, changes)
addon.replay(ctx)
const firstText = diff => {
  if (diff.type === 'text') return diff.objectId
  for (const key of Object.keys(diff.props || {})) for (const id of Object.keys(diff.props[key])) if (diff.props[key][id].objectId) { const r = firstText(diff.props[key][id]); if (r) return r }
  return null
}
const objectId = firstText(materialize(addon.fetchIR(ctx, true)).diffs)
const [ctr, actorHex] = objectId.split('@')
const actor = new Uint8Array(Buffer.from(actorHex, 'hex'))
const t = { text: [], textAgain: [], fetch: [], materialize: [], fold: [] }
let chars = 0, length = 0
for (let r = 0; r < reps + 2; r++) {
  addon.replay(ctx)
  const t0 = ms()
  const a = addon.objectText(ctx, Number(ctr), actor)
  const t1 = ms()
  const a2 = addon.objectText(ctx, Number(ctr), actor)
  const t2 = ms()
  addon.replay(ctx)
  const t3 = ms()
  const ir = addon.fetchIR(ctx, true)
  const t4 = ms()
  const patch = materialize(ir)
  const t5 = ms()
  const b = textFromPatch(patch, objectId)
  const t6 = ms()
  if (a.text !== b.text || a2.text !== b.text || a.length !== b.length) throw new Error('the engine\'s string differs from the folded patch')
  if (r >= 2) { t.text.push(t1 - t0); t.textAgain.push(t2 - t1); t.fetch.push(t4 - t3); t.materialize.push(t5 - t4); t.fold.push(t6 - t5) }
  chars = a.text.length; length = a.length
}
const med = a => a.slice().sort((x, y) => x - y)[Math.floor(a.length / 2)]
const spread = a => [Math.min(...a), Math.max(...a)]
const m = {}, mm = {}
for (const k of Object.keys(t)) { m[k] = med(t[k]); mm[k] = spread(t[k]) }
console.log(JSON.stringify({ n_ops: nOps, n_changes: n, reps, objectId, utf16_units: chars, elements: length, ms: m, min_max_ms: mm,
  getText_engine_ms: m.text, getPatch_materialize_fold_ms: m.fetch + m.materialize + m.fold }))
