// What the sync message after a keystroke and half of Automerge.merge cost through the JS host: after every one-change
// Backend.applyChanges onto a large engine-built state,
//   (a) the first Backend.getChanges(state, previous heads)          -- every applyChanges makes a new state: per-state indexes start over
//   (b) Backend.getChangesAdded(behind, state)                       -- two states one change apart: a second lineage gets every change a round later
// are timed. (b) needs either this tree's engine path or the reference backend (the hydrating path of earlier trees): where neither is
// there the row says so instead of a time.
//
//   python -c "from automerge_classic_amd import loggen; loggen.config('c4_text_single', 1.0, False).save('/tmp/c4.bin')"
//   node automerge_classic_amd/js/bench_graph_queries.js /tmp/c4.bin [calls = 12] [directory of the index.js to time = this one]
'use strict'
const fs = require('fs')
const path = require('path')
const Backend = require(path.join(process.argv[4] || __dirname, 'index.js'))

const buf = fs.readFileSync(process.argv[2])
const calls = parseInt(process.argv[3] || '12')
const n = buf.readUInt32LE(0)
const offs = []
for (let i = 0; i <= n; i++) offs.push(Number(buf.readBigUInt64LE(12 + 8 * i)))
const base = 12 + 8 * (n + 1)
const changes = []
for (let i = 0; i < n; i++) changes.push(new Uint8Array(buf.buffer, buf.byteOffset + base + offs[i], offs[i + 1] - offs[i]))

const ms = () => Number(process.hrtime.bigint()) / 1e6
const median = a => { const s = a.slice().sort((x, y) => x - y); return s[Math.floor(s.length / 2)] }
const first = n - calls
// two lineages from the same changes, one call apart: `behind` gets every change one round after `state`
const empty = () => ({ state: { changes: [], queue: [] }, heads: [] })
let state = Backend.applyChanges(empty(), changes.slice(0, first))[0]
let behind = Backend.applyChanges(empty(), changes.slice(0, first))[0]
const apply = [], since = [], added = []
let addedError = null
for (let j = 0; j < calls; j++) {
  const prevHeads = Backend.getHeads(state)
  let t0 = ms()
  state = Backend.applyChanges(state, [changes[first + j]])[0]
  apply.push(ms() - t0)
  t0 = ms()
  const got = Backend.getChanges(state, prevHeads)
  since.push(ms() - t0)
  if (got.length !== 1 || got[0] !== changes[first + j]) throw new Error('getChanges(previous heads) is not the change just applied')
  if (addedError === null) {
    try {
      t0 = ms()
      const more = Backend.getChangesAdded(behind, state)
      added.push(ms() - t0)
      if (more.length !== 1 || more[0] !== changes[first + j]) throw new Error('getChangesAdded is not the change just applied')
    } catch (e) {
      if (!/Cannot find module/.test(e.message)) throw e
      addedError = 'needs the reference backend (the states would be hydrated): not installed here'
    }
  }
  if (addedError === null) behind = Backend.applyChanges(behind, [changes[first + j]])[0]
}
console.log(JSON.stringify({
  tree: process.argv[4] || __dirname, n_changes: n, calls,
  apply_ms: { first: apply[0], median: median(apply.slice(1)) },
  get_changes_prev_heads_ms: { first: since[0], median: median(since.slice(1)), min: Math.min(...since) },
  get_changes_added_ms: addedError || { first: added[0], median: median(added.slice(1)), min: Math.min(...added) },
  counters: Backend._counters
}))
