// TEST INFRASTRUCTURE (build container only: it needs the live reference): the hash-graph queries of tests/test_hash_graph.py and
// tests/test_js_graph_queries.py. Histories made by the reference FRONTEND (Automerge.change / applyChanges between replicas) are
// delivered to the reference's backend batch by batch, and its answers are recorded as lists of hashes.
// Writes tests/golden/graph/queries.json: per history
//   changes        the delivery, in order (base64); hashes: their hashes; batches: how many of them each Backend.applyChanges call got
//   applied, queued, heads   Backend.getAllChanges order / the queue / getHeads of the final state, as hashes
//   get_changes    [{ have, result } | { have, error }]           Backend.getChanges(state, have)
//   change_by_hash [{ hash, found }]                              Backend.getChangeByHash(state, hash) !== undefined
//   missing_deps   [{ heads, result }]                            Backend.getMissingDeps(state, heads)
//   changes_added  [{ name, first, second, result, merged_patch }]
//                  first / second: indexes into `changes` of the two states' deliveries (each one applyChanges call onto init());
//                  result = Backend.getChangesAdded(stateFirst, stateSecond); merged_patch = JSON.stringify(getPatch) of
//                  applyChanges(stateFirst, result). stateFirst has applied everything it was given (nothing queued)
// Data only.
//   NODE_PATH=oracle/js_shims/node_modules node tools/fixtures/make_graph_queries.js
const path = require('path')
const fs = require('fs')
const ROOT = path.join(__dirname, '..', '..')
const { loadBackend } = require(path.join(ROOT, 'oracle', 'js', 'ref_loader'))
const ref = loadBackend()
const { Backend, columnar } = ref
const Automerge = ref.Automerge()
const { decodeChange } = columnar
const id = d => d.repeat(32 / d.length)
const b64 = u8 => Buffer.from(u8.buffer, u8.byteOffset, u8.byteLength).toString('base64')
const hashOf = c => decodeChange(c).hash
const UNKNOWN = 'ab'.repeat(32), UNKNOWN2 = '0f'.repeat(32)

class Peer {
  constructor(actor, all) { this.doc = Automerge.init(actor); this.all = all }
  change(fn) {
    this.doc = Automerge.change(this.doc, { time: 0 }, fn)
    const c = Automerge.getLastLocalChange(this.doc)
    this.all.push(c)
    return c
  }
  see(other) { this.doc = Automerge.merge(this.doc, other.doc) }
}

// ---- the histories: every change in the order it was made (a causal order) ----
function linear() {
  const all = [], a = new Peer(id('1'), all)
  a.change(d => { d.text = new Automerge.Text('ab'); d.n = 0 })
  for (let k = 1; k < 12; k++) a.change(d => { d.n = k; d.text.insertAt(k, String.fromCharCode(97 + k)) })
  return all
}
function diamonds() {
  const all = [], a = new Peer(id('2'), all), b = new Peer(id('5'), all), c = new Peer(id('8'), all)
  a.change(d => { d.text = new Automerge.Text('base'); d.votes = {} })
  b.see(a); c.see(a)
  for (let r = 0; r < 3; r++) {
    a.change(d => { d.votes['a' + r] = r })
    b.change(d => { d.text.insertAt(1, 'b') })
    if (r !== 1) b.change(d => { d.votes['b' + r] = r })
    c.change(d => { d.text.insertAt(2, 'c') })
    a.see(b)                                    // a diamond: a's next change has two parents
    a.change(d => { d.votes.merged = 'ab' + r })
    c.see(a); b.see(c)                          // repeated merges: c and b catch up at different points
    c.change(d => { d.votes['c' + r] = r })
    a.see(c)
  }
  a.change(d => { d.done = true })
  return all
}
function sixConcurrent() {
  const all = [], first = new Peer(id('1'), all)
  first.change(d => { d.list = []; d.who = {} })
  const peers = ['3', '4', '6', '7', '9', 'c'].map(x => { const p = new Peer(id(x), all); p.see(first); return p })
  for (let r = 0; r < 2; r++) peers.forEach((p, k) => p.change(d => { d.who['p' + k] = r; d.list.push(k * 10 + r) }))
  for (const p of peers) first.see(p)
  first.change(d => { d.merged = true })
  return all
}

const ancestorsOf = (metaByHash, h) => {
  const seen = new Set(), stack = [h]
  while (stack.length) { const x = stack.pop(); if (!seen.has(x)) { seen.add(x); stack.push(...metaByHash.get(x).deps) } }
  return seen
}

function record(name, note, delivery, batches, opts = {}) {
  let state = Backend.init()
  let at = 0
  for (const n of batches) { state = Backend.applyChanges(state, delivery.slice(at, at + n))[0]; at += n }
  if (at !== delivery.length) throw new Error(name + ': the batches do not cover the delivery')
  const hashes = delivery.map(hashOf)
  const meta = new Map(delivery.map(c => { const m = decodeChange(c); return [m.hash, m] }))
  const applied = Backend.getAllChanges(state).map(hashOf)
  const queued = state.state.queue.map(c => c.hash)
  const heads = Backend.getHeads(state)
  const out = { name, note, changes: delivery.map(b64), hashes, batches, applied, queued, heads, get_changes: [], change_by_hash: [], missing_deps: [], changes_added: [] }
  const ask = have => {
    try { out.get_changes.push({ have, result: Backend.getChanges(state, have).map(hashOf) }) } catch (e) { out.get_changes.push({ have, error: e.message }) }
  }
  ask([])
  ask(heads)
  const step = opts.singleStep || 4
  const singles = applied.filter((_, k) => k % step === 0 || k === applied.length - 1)
  for (const h of singles) ask([h])
  // pairs of concurrent hashes, and a hash together with one of its ancestors (the walk over dependents then meets a change twice or
  // misses a dependency: the second branch)
  const anc = new Map(applied.map(h => [h, ancestorsOf(meta, h)]))
  let pairs = 0, withAncestor = 0
  for (let i = 0; i < applied.length && pairs < 4; i++)
    for (let j = i + 1; j < applied.length && pairs < 4; j += 3)
      if (!anc.get(applied[i]).has(applied[j]) && !anc.get(applied[j]).has(applied[i])) { ask([applied[i], applied[j]]); ask([applied[j], applied[i]]); pairs++ }
  for (let i = applied.length - 1; i > 0 && withAncestor < 3; i -= 2) {
    const a = Array.from(anc.get(applied[i])).filter(h => h !== applied[i])
    if (a.length) { ask([applied[i], a[a.length - 1]]); ask([a[0], applied[i]]); withAncestor++ }
  }
  ask([UNKNOWN])
  ask([applied[0], UNKNOWN, UNKNOWN2])
  for (const q of queued.slice(0, 2)) ask([q])
  for (const h of [applied[0], applied[applied.length - 1], ...queued.slice(0, 2), UNKNOWN])
    out.change_by_hash.push({ hash: h, found: Backend.getChangeByHash(state, h) !== undefined })
  for (const hs of [[], heads, [UNKNOWN], [applied[0], UNKNOWN2, UNKNOWN], queued.slice(0, 1), queued.concat([UNKNOWN, heads[0]])])
    out.missing_deps.push({ heads: hs, result: Backend.getMissingDeps(state, hs) })
  for (const [pairName, first, second] of opts.pairs || []) {
    const s1 = first.length ? Backend.applyChanges(Backend.init(), first.map(i => delivery[i]))[0] : Backend.init()
    const s2 = second.length ? Backend.applyChanges(Backend.init(), second.map(i => delivery[i]))[0] : Backend.init()
    if (s1.state.queue.length) throw new Error(name + ' ' + pairName + ': the first state must have applied all it was given')
    const added = Backend.getChangesAdded(s1, s2)
    const merged = added.length ? Backend.applyChanges(s1, added)[0] : s1
    out.changes_added.push({ name: pairName, first, second, result: added.map(hashOf), merged_patch: JSON.stringify(Backend.getPatch(merged)) })
  }
  return out
}

const range = (a, b) => Array.from({ length: b - a }, (_, k) => a + k)
const histories = []
{
  const all = linear(), n = all.length
  histories.push(record('linear', 'one actor, every change on the one before', all, [3, 1, 1, 2, 1, 4], {
    singleStep: 1,
    pairs: [['equal', range(0, n), range(0, n)], ['ahead', range(0, 5), range(0, n)], ['behind', range(0, n), range(0, 5)], ['empty_other', [], range(0, n)],
      ['one_apart', range(0, n - 1), range(0, n)]]
  }))
}
{
  const all = diamonds(), n = all.length
  const meta = new Map(all.map(c => { const m = decodeChange(c); return [m.hash, m] }))
  const hashes = all.map(hashOf)
  const closure = i => range(0, n).filter(k => ancestorsOf(meta, hashes[i]).has(hashes[k]))
  // two states that diverge both ways: the histories of two concurrent changes, the pair that knows most
  let b = null, c = null
  for (let i = 0; i < n; i++)
    for (let j = i + 1; j < n; j++) {
      const ci = closure(i), cj = closure(j)
      if (!ci.includes(j) && !cj.includes(i) && (!b || Math.min(ci.length, cj.length) > Math.min(b.length, c.length))) { b = ci; c = cj }
    }
  const a5 = closure(Math.floor(n / 2))
  histories.push(record('diamonds', 'three actors: changes with two parents, merges at different points, three rounds', all, [4, 2, 1, 3, 1, 1, n - 12], {
    singleStep: 2,
    pairs: [['equal', range(0, n), range(0, n)], ['ahead', a5, range(0, n)], ['diverged_bc', b, c], ['diverged_cb', c, b], ['empty_other', [], range(0, n)],
      ['other_superset', range(0, n), a5]]
  }))
  // the same history with one early change of the second actor withheld: it and everything behind it stays queued
  const withheld = range(0, n).find(k => decodeChange(all[k]).actor === id('5') && decodeChange(all[k]).seq === 4)
  const delivery = all.filter((_, k) => k !== withheld)
  const m = delivery.length
  histories.push(record('withheld', `the diamonds history without its change ${withheld} (second actor, seq 4): what depends on it is queued`, delivery, [5, 3, m - 8], {
    pairs: [['ahead_with_queue', range(0, 3), range(0, m)], ['empty_other', [], range(0, m)]]
  }))
}
{
  const all = sixConcurrent(), n = all.length
  histories.push(record('six_concurrent', 'six actors, two changes each on one base, merged by the first actor at the end', all, [1, 6, 6, 1], {
    pairs: [['equal', range(0, n), range(0, n)], ['ahead', range(0, 7), range(0, n)], ['diverged_a', [0, 1, 2, 3, 7, 8, 9], [0, 4, 5, 6, 10, 11, 12]],
      ['diverged_b', [0, 4, 5, 6, 10, 11, 12], [0, 1, 2, 3, 7, 8, 9]], ['empty_other', [], range(0, n)], ['other_superset', range(0, n), range(0, 7)]]
  }))
  // duplicates: two inside the first call, two changes of the first call again in the second
  const delivery = [all[0], all[1], all[1], all[2], all[3], all[0], all[4], all[5], all[6]].concat([all[2], all[7], all[8], all[5]], all.slice(9))
  const m = delivery.length
  histories.push(record('duplicates', 'the six-actor history with changes delivered twice: inside one call and again in a later call', delivery, [9, 4, m - 13], {
    pairs: [['ahead', range(0, 9), range(0, m)], ['equal_with_dups', range(0, m), range(0, m)]]
  }))
}

const dir = path.join(ROOT, 'tests', 'golden', 'graph')
fs.mkdirSync(dir, { recursive: true })
const file = path.join(dir, 'queries.json')
fs.writeFileSync(file, JSON.stringify({ note: 'tools/fixtures/make_graph_queries.js: hash-graph queries answered by the reference backend', unknown: UNKNOWN, histories }))
for (const h of histories) {
  const second = h.get_changes.filter(q => q.result && q.have.length && q.result.length && h.applied.filter(x => q.result.includes(x)).join() === q.result.join()).length
  console.log(h.name, 'changes', h.changes.length, 'applied', h.applied.length, 'queued', h.queued.length, 'heads', h.heads.length, 'getChanges', h.get_changes.length,
    '(answers in application order:', second + ')', 'errors', h.get_changes.filter(q => q.error).length, 'pairs', h.changes_added.map(p => p.name + ':' + p.result.length).join(' '))
}
console.log(file, fs.statSync(file).size, 'bytes')
