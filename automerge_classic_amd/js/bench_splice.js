// One character typed at a position in the middle of the headline document's Text, through the JS host: spliceText served by the engine
// (am355_text_splice: the positions resolved on the device) against the same call on the JS path of index.js -- the whole-document patch
// fetched and materialised (fetchIR + materialize.js), folded into elemIds and preds, the request handed to applyLocalChange. Both go
// on from the state the other left, alternating. (A host with a frontend document pays applyPatch and Automerge.change on top of the
// fetch and the materialisation; that route needs the reference's frontend and is not timed here.)
//
//   python -c "from automerge_classic_amd import loggen; loggen.config('c4_text_single', 1.0, False).save('/tmp/c4.bin')"
//   node automerge_classic_amd/js/bench_splice.js /tmp/c4.bin [reps]
//
// Log file layout (little endian): u32 n_changes, u64 n_ops, u64 offsets[n+1], arena.
'use strict'
const fs = require('fs')
const path = require('path')
const Backend = require(path.join(__dirname, 'index.js'))

const buf = fs.readFileSync(process.argv[2])
const reps = parseInt(process.argv[3] || '9')
const n = buf.readUInt32LE(0)
const nOps = Number(buf.readBigUInt64LE(4))
const offs = []
for (let i = 0; i <= n; i++) offs.push(Number(buf.readBigUInt64LE(12 + 8 * i)))
const base = 12 + 8 * (n + 1)
const changes = []
for (let i = 0; i < n; i++) changes.push(new Uint8Array(buf.buffer, buf.byteOffset + base + offs[i], offs[i + 1] - offs[i]))

const ms = () => Number(process.hrtime.bigint()) / 1e6
const firstText = diff => {
  if (diff.type === 'text') return diff.objectId
  for (const key of Object.keys(diff.props || {})) for (const id of Object.keys(diff.props[key])) if (diff.props[key][id].objectId) { const r = firstText(diff.props[key][id]); if (r) return r }
  return null
}
let [state, patch] = Backend.applyChanges({ state: { changes: [], queue: [] }, heads: [] }, changes)
const objectId = firstText(patch.diffs)
const actor = 'e5'.repeat(16)
const t = { engine: [], jsPath: [], locate: [] }
let length = Backend.locateText(state, objectId, 0, 0).length
for (let r = 0; r < reps + 2; r++) {
  const mid = length >> 1
  const t0 = ms()
  Backend.locateText(state, objectId, mid - 1, 1)
  const t1 = ms()
  state = Backend.spliceText(state, objectId, mid, 0, 'x', { actor, time: r })[0]
  const t2 = ms()
  Backend._setSpliceOnEngine(false)
  const t3 = ms()
  state = Backend.spliceText(state, objectId, mid, 0, 'y', { actor, time: r })[0]
  const t4 = ms()
  Backend._setSpliceOnEngine(true)
  length += 2
  if (r >= 2) { t.locate.push(t1 - t0); t.engine.push(t2 - t1); t.jsPath.push(t4 - t3) }
}
if (Backend.locateText(state, objectId, 0, 0).length !== length) throw new Error('the Text did not grow by the characters typed')
const c = Backend._counters
if (c.gpuSplice !== reps + 2 || c.spliceFallbacks !== reps + 2 || c.hydrations !== 0 || c.localFallbacks !== 0) throw new Error('not served as meant: ' + JSON.stringify(c))
const med = a => a.slice().sort((x, y) => x - y)[Math.floor(a.length / 2)]
const m = {}, mm = {}
for (const k of Object.keys(t)) { m[k] = med(t[k]); mm[k] = [Math.min(...t[k]), Math.max(...t[k])] }
console.log(JSON.stringify({ n_ops: nOps, n_changes: n, reps, objectId, elements: length, ms: m, min_max_ms: mm,
  spliceText_engine_ms: m.engine, spliceText_js_path_ms: m.jsPath, counters: c }))
