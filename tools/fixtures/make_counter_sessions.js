// TEST INFRASTRUCTURE (build container only: it needs the live reference): the sessions of tests/test_resident_counters.py -- calls whose
// batch INCREMENTS counters on map keys (am355_set_resident_counters), shaped by the reference FRONTEND (Automerge.change: the op shapes
// applications produce). No generator kind of loggen increments a counter inside a session.
// Writes tests/golden/resident/counters.json: per session the batches (changes in base64), the reference's incremental patch per call,
// its whole patch at the end, and per call its kind -- what the test expects of the path that serves it:
//   setup        nothing asserted about the path
//   inc          increments of map counters only
//   list+inc     an increment and list rows in one batch
//   beside       increments beside plain map rows (or a counter made and incremented at once): the map half serves them
//   beside+list  the same beside list rows (a push of a map: with am355_set_resident_new_objects)
//   declined     a key with conflicting values, one of them the counter incremented
//   listinc      a counter inside a list incremented
// Data only. Then checks through tests/oracle_lib.py (OracleSession) that the sequential oracle reproduces every recorded patch, and
// prints the outcome per session; a session the oracle cannot follow is dropped from the file.
//   NODE_PATH=oracle/js_shims/node_modules node tools/fixtures/make_counter_sessions.js
const path = require('path')
const fs = require('fs')
const { spawnSync } = require('child_process')
const ROOT = path.join(__dirname, '..', '..')
const { loadBackend } = require(path.join(ROOT, 'oracle', 'js', 'ref_loader'))
const ref = loadBackend()
const { Backend, columnar } = ref
const Automerge = ref.Automerge()
const { decodeChange, encodeChange } = columnar
const id = d => d.repeat(32)
const b64 = u8 => Buffer.from(u8.buffer, u8.byteOffset, u8.byteLength).toString('base64')
const rowsOf = c => decodeChange(c).ops.reduce((n, op) => n + (op.values ? op.values.length : 1), 0)

// One author's replica and the changes it has made or seen; `change` returns the binary change of one Automerge.change
class Peer {
  constructor(actor, changes = []) {
    this.doc = Automerge.init(actor)
    if (changes.length) this.see(changes)
  }
  change(fn) {
    this.doc = Automerge.change(this.doc, { time: 0 }, fn)
    return Automerge.getLastLocalChange(this.doc)
  }
  see(changes) { this.doc = Automerge.applyChanges(this.doc, changes)[0] }
}

// the op id of the `set` of `key` in _root among the ops of change c
function rootOpId(c, key) {
  const d = decodeChange(c)
  let ctr = d.startOp
  for (const op of d.ops) {
    if (op.obj === '_root' && op.key === key) return `${ctr}@${d.actor}`
    ctr += op.values ? op.values.length : 1
  }
  throw new Error('no op on ' + key)
}

// a session: [{ batch: [changes], kind }]
function record(name, note, calls) {
  let state = Backend.init()
  const patches = []
  for (const call of calls) {
    const r = Backend.applyChanges(state, call.batch)
    state = r[0]
    patches.push(JSON.stringify(r[1]))
  }
  const rows = calls.map(call => call.batch.reduce((n, c) => n + rowsOf(c), 0))
  return { name, note, batches: calls.map(call => call.batch.map(b64)), kinds: calls.map(call => call.kind || 'setup'), rows, patches,
    whole_patch: JSON.stringify(Backend.getPatch(state)) }
}

const A = id('7'), B = id('9')
const TEXT = 't'.repeat(35) + 'u'.repeat(35)   // (a list longer than one wavefront)

// two authors the document knows from the first call on, a Text of 70 characters and what `fill` adds
function pair(fill, a = new Peer(A), actorB = B) {
  const setup = a.change(d => { d.text = new Automerge.Text(TEXT); fill(d) })
  const b = new Peer(actorB, [setup])
  const hello = b.change(d => { d.hello = 1 })
  a.see([hello])
  return { a, b, first: { batch: [setup, hello] } }
}

function plain() {
  const { a, b, first } = pair(d => {
    for (let k = 0; k < 64; k++) d['key' + String(k).padStart(2, '0')] = k   // (with the keys below: more than one wavefront of records in _root)
    d.a_key_of_sixteen_bytes_and_more_1 = new Automerge.Counter(0)   // (two keys that agree in their first sixteen bytes)
    d.a_key_of_sixteen_bytes_and_more_2 = 'two'
    d.votes = new Automerge.Counter(0)
    d.zeta = new Automerge.Counter(7)
    d.big = new Automerge.Counter(4294967290)
    d.stats = { hits: new Automerge.Counter(0), misses: 3 }   // (object index != 0, map_begin != 0)
  })
  const calls = [first]
  const one = (peer, other, fn, kind = 'inc') => { const c = peer.change(fn); other.see([c]); calls.push({ batch: [c], kind }) }
  one(a, b, d => { d.votes.increment() })                       // the first increment: flag 0 -> counter
  one(a, b, d => { d.votes.increment(4) })                      // a second one
  one(b, a, d => { d.votes.decrement(9) })                      // below zero
  one(a, b, d => { d.big.increment(10) })                       // a total past 2^32
  {
    // two increments of one counter in one change, both naming the counter as their pred (encodeChange: the frontend names the first
    // increment as the second one's pred, which the reference's backend rejects)
    const last = decodeChange(calls[calls.length - 1].batch[0]), zeta = rootOpId(first.batch[0], 'zeta')
    const startOp = last.startOp + rowsOf(calls[calls.length - 1].batch[0])
    const c = encodeChange({ actor: A, seq: Automerge.getHistory(a.doc).filter(h => h.change.actor === A).length + 1, startOp, time: 0, message: '', deps: [last.hash],
      ops: [{ action: 'inc', obj: '_root', key: 'zeta', value: 1, pred: [zeta] }, { action: 'inc', obj: '_root', key: 'zeta', value: 2, pred: [zeta] }] })
    a.see([c]); b.see([c])
    calls.push({ batch: [c], kind: 'inc' })
  }
  one(b, a, d => { d.a_key_of_sixteen_bytes_and_more_1.increment(3) })
  one(a, b, d => { d.stats.hits.increment() })                  // inside a nested map
  const ca = a.change(d => { d.votes.increment(100) }), cb = b.change(d => { d.votes.increment(1000); d.stats.hits.increment(5) })
  a.see([cb]); b.see([ca])
  calls.push({ batch: [ca, cb], kind: 'inc' })                  // both authors, concurrent, in one batch
  one(a, b, d => { d.zeta.increment(); d.text.insertAt(35, 'x', 'y', 'z') }, 'list+inc')   // an increment and typing in one change
  const many = []
  for (let k = 0; k < 40; k++) many.push(a.change(d => { [d.votes, d.zeta, d.big, d.stats.hits][k % 4].increment(k) }))
  b.see(many)
  calls.push({ batch: many, kind: 'inc' })                      // 40 one-increment changes
  one(b, a, d => { d.text.deleteAt(3); d.votes.increment() }, 'list+inc')
  return record('plain', 'a root map of 70 keys, counters on four of them and one in a nested map: first increments, decrements, a total past 2^32, ' +
    'two increments in one change, concurrent increments, an increment beside typing, 40 changes in one call', calls)
}

function beside() {
  const { a, first } = pair(d => { d.votes = new Automerge.Counter(0); d.title = 'a' })
  const calls = [first]
  calls.push({ batch: [a.change(d => { d.votes.increment(); d.title2 = 'x' })], kind: 'beside' })
  calls.push({ batch: [a.change(d => { d.c = new Automerge.Counter(1); d.c.increment() })], kind: 'beside' })
  calls.push({ batch: [a.change(d => { d.c.increment(2) })], kind: 'inc' })
  return record('beside', 'an increment beside a key assigned; a counter made and incremented in one change', calls)
}

function besidePush() {
  const { a, first } = pair(d => { d.votes = new Automerge.Counter(0); d.cards = [] })
  const calls = [first]
  calls.push({ batch: [a.change(d => { d.votes.increment(2); d.cards.push({ x: 1 }) })], kind: 'beside+list' })
  calls.push({ batch: [a.change(d => { d.votes.increment(3) })], kind: 'inc' })
  return record('beside_push', 'an increment beside a pushed map (with am355_set_resident_new_objects: list merge in place, then the map half)', calls)
}

function declined() {
  const { a, b, first } = pair(d => { d.list = [new Automerge.Counter(1), 2] })
  const calls = [first]
  // B's value of the key is the counter and wins the conflict (equal op counters, the greater actor): B's frontend increments it
  const ca = a.change(d => { d.x = 'text' }), cb = b.change(d => { d.x = new Automerge.Counter(5) })
  a.see([cb]); b.see([ca])
  calls.push({ batch: [ca, cb] })
  calls.push({ batch: [b.change(d => { d.x.increment(2) })], kind: 'declined' })
  calls.push({ batch: [a.change(d => { d.list[0].increment(4) })], kind: 'listinc' })
  return record('declined', 'a key with two conflicting values, one of them a counter, incremented; a counter inside a list incremented', calls)
}

function gone() {
  const { a, b, first } = pair(d => { d.c = new Automerge.Counter(3); d.keep = new Automerge.Counter(1) })
  const calls = [first]
  const del = a.change(d => { delete d.c }), inc = b.change(d => { d.c.increment(5) })
  calls.push({ batch: [del] })
  calls.push({ batch: [inc], kind: 'inc' })
  a.see([inc])
  calls.push({ batch: [a.change(d => { d.keep.increment() })], kind: 'inc' })
  return record('gone', 'a counter deleted by one author and incremented concurrently by the other, the deletion delivered first', calls)
}

function newcomer() {
  // the newcomer's id sorts in front of both known authors': every kept rank moves
  const { a, first } = pair(d => { d.votes = new Automerge.Counter(0) }, new Peer(id('c')), id('e'))
  const calls = [first]
  calls.push({ batch: [a.change(d => { d.votes.increment() })], kind: 'inc' })   // (last_inc holds a rank the rewrite must move)
  const n = new Peer(id('3'), first.batch.concat(calls[1].batch))
  const c = n.change(d => { d.votes.increment(10) })
  calls.push({ batch: [c], kind: 'inc' })
  a.see([c])
  calls.push({ batch: [a.change(d => { d.votes.increment(100) })], kind: 'inc' })
  return record('newcomer', 'a third author, whose id sorts in front of both known ones, increments as their first change', calls)
}

let sessions = []
for (const make of [plain, beside, besidePush, declined, gone, newcomer]) {
  try { sessions.push(make()) } catch (e) { console.log(make.name, 'dropped: the reference rejects it:', e.message) }
}
const dir = path.join(ROOT, 'tests', 'golden', 'resident')
fs.mkdirSync(dir, { recursive: true })
const file = path.join(dir, 'counters.json')
const write = () => fs.writeFileSync(file, JSON.stringify({ note: 'tools/fixtures/make_counter_sessions.js: reference frontend sessions whose calls increment counters', sessions }))
write()

// the sequential oracle against the file just written: one line per session, `name ok` or `name FAILS ...`
const check = `
import base64, json, sys
sys.path.insert(0, ${JSON.stringify(path.join(ROOT, 'tests'))}); sys.path.insert(0, ${JSON.stringify(ROOT)})
import oracle_lib
from test_apply_vectors import same_patch
from test_apply_engine import _ordered
for s in json.load(open(${JSON.stringify(file)}))["sessions"]:
    session, bad = oracle_lib.OracleSession(), None
    try:
        for i, (batch, want) in enumerate(zip(s["batches"], s["patches"])):
            if not same_patch(session.apply([base64.b64decode(c) for c in batch]), want):
                bad = "call %d" % i
                break
        if bad is None and dict(_ordered(session.patch_json()))["diffs"] != dict(_ordered(s["whole_patch"]))["diffs"]:
            bad = "getPatch at the end"
    except Exception as e:
        bad = repr(e)
    finally:
        session.close()
    print(s["name"], "ok" if bad is None else "FAILS " + bad)
`
const r = spawnSync('python3', ['-c', check], { encoding: 'utf8' })
if (r.status !== 0) { console.log(r.stdout, r.stderr); throw new Error('the oracle check did not run') }
const failed = new Set()
for (const line of r.stdout.trim().split('\n')) {
  const [name, verdict] = line.split(' ')
  if (verdict !== 'ok') failed.add(name)
  console.log('oracle:', line)
}
if (failed.size) { sessions = sessions.filter(s => !failed.has(s.name)); write() }
for (const s of sessions) console.log(s.name, s.batches.length, 'calls, rows', s.rows.join(' '), '|', s.kinds.join(' '))
console.log(file, fs.statSync(file).size, 'bytes')
