// TEST INFRASTRUCTURE (build container only: it needs the live reference): the sessions of tests/test_text_read.py and
// js/test_text_read.js -- documents whose Text objects are read on the device (am355_object_text), shaped by the reference FRONTEND
// (Automerge.change: the op shapes applications produce) and a few hand-encoded changes where the frontend makes none.
// Writes tests/golden/text/text_reads.json: per session the batches (changes in base64), the reference backend's incremental patch per call,
// and after every call, for every Text object of the document, {objectId, string: text.toString(), length: text.length} as the state of
// the reference frontend's Automerge.applyChanges shows them; at the end the reference's save bytes.
// Data only. Then checks through tests/oracle_lib.py (OracleSession) that the sequential oracle reproduces every recorded patch, and
// prints the outcome per session; a session the oracle cannot follow is dropped from the file.
//   NODE_PATH=oracle/js_shims/node_modules node tools/fixtures/make_text_reads.js
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

class Peer {
  constructor(actor, changes = []) {
    this.actor = actor
    this.doc = Automerge.init(actor)
    if (changes.length) this.see(changes)
  }
  change(fn) {
    this.doc = Automerge.change(this.doc, { time: 0 }, fn)
    return Automerge.getLastLocalChange(this.doc)
  }
  see(changes) { this.doc = Automerge.applyChanges(this.doc, changes)[0] }
}

// every Text object reachable in a frontend document
function textsOf(node, out) {
  if (node instanceof Automerge.Text) {
    out.push({ objectId: Automerge.getObjectId(node), string: node.toString(), length: node.length })
    for (let i = 0; i < node.length; i++) textsOf(node.get(i), out)
  } else if (node instanceof Automerge.Counter || node instanceof Date || node instanceof Uint8Array) {
    // no children
  } else if (Array.isArray(node)) {
    for (const v of node) textsOf(v, out)
  } else if (node && typeof node === 'object') {
    for (const k of Object.keys(node)) textsOf(node[k], out)
  }
  return out
}

// a session: [[changes of a call]]
function record(name, note, batches) {
  let state = Backend.init(), view = Automerge.init(id('f'))
  const patches = [], texts = []
  for (const batch of batches) {
    const r = Backend.applyChanges(state, batch)
    state = r[0]
    patches.push(JSON.stringify(r[1]))
    view = Automerge.applyChanges(view, batch)[0]
    texts.push(textsOf(view, []).sort((x, y) => (x.objectId < y.objectId ? -1 : 1)))
  }
  return { name, note, batches: batches.map(b => b.map(b64)), rows: batches.map(b => b.reduce((n, c) => n + rowsOf(c), 0)), patches, texts,
    whole_patch: JSON.stringify(Backend.getPatch(state)), save: b64(Backend.save(state)) }
}

const A = id('2'), B = id('7'), C = id('c')
// everybody sees what the others made in a round; the round is one call
function round(peers, fns) {
  const made = peers.map((p, i) => (fns[i] ? p.change(fns[i]) : null))
  peers.forEach((p, i) => p.see(made.filter((c, j) => c && j !== i)))
  return made.filter(c => c)
}

function typed() {
  const a = new Peer(A)
  const setup = a.change(d => { d.text = new Automerge.Text('The quick brown fox jumps over the lazy dog. ') })
  const b = new Peer(B, [setup]), c = new Peer(C, [setup])
  const peers = [a, b, c], batches = [[setup]]
  const MIX = ['a', 'é', '€', '😀', 'z', '中', 'ß', 'q', '🌍', 'あ']   // 1, 2, 3 and 4 bytes inside one run
  for (let r = 0; r < 6; r++) {
    batches.push(round(peers, peers.map((p, i) => d => {
      const at = (7 * r + 11 * i) % d.text.length
      const run = []
      for (let k = 0; k < 12 + i; k++) run.push(i === 0 ? String.fromCharCode(97 + (k + r) % 26) : MIX[(k + r + i) % MIX.length])
      d.text.insertAt(at, ...run)
      if (r % 2 === i % 2) d.text.deleteAt((at + 5) % (d.text.length - 3), 3)
    })))
  }
  // one author alone, call by call: a keystroke, a pasted word, a deletion (the in-place merges)
  for (let k = 0; k < 6; k++) {
    const ch = a.change(d => {
      if (k % 3 === 0) d.text.insertAt(k * 5, 'K')
      else if (k % 3 === 1) d.text.insertAt(k * 3, ...'päste€'.split(''))
      else d.text.deleteAt(k * 2, 2)
    })
    b.see([ch]); c.see([ch])
    batches.push([ch])
  }
  return record('typed', 'three authors typing concurrently with deletions; runs that mix characters of 1, 2, 3 and 4 bytes; then single keystrokes', batches)
}

function conflicts() {
  const a = new Peer(A)
  const setup = a.change(d => { d.text = new Automerge.Text('abcdefghijklmnopqrstuvwxyz') })
  const b = new Peer(B, [setup]), c = new Peer(C, [setup])
  const peers = [a, b, c], batches = [[setup]]
  // in the middle of the typed run
  batches.push(round(peers, [d => { d.text.set(10, 'X') }, d => { d.text.set(10, 'Y') }]))
  // on the last element of the typed run
  batches.push(round(peers, [d => { d.text.set(25, '1') }, d => { d.text.set(25, '2') }]))
  // three concurrent assignments to one element
  batches.push(round(peers, [d => { d.text.set(3, 'é') }, d => { d.text.set(3, '€') }, d => { d.text.set(3, 'w') }]))
  // a conflict whose winner is a number (the greater actor)
  batches.push(round(peers, [d => { d.text.set(5, 'five') }, null, d => { d.text.set(5, 5) }]))
  // typing goes on behind the conflicts; a conflict resolved by a later assignment
  batches.push(round(peers, [d => { d.text.insertAt(26, ...'-end') }, d => { d.text.set(10, 'Z') }]))
  batches.push(round(peers, [d => { d.text.deleteAt(25) }, d => { d.text.set(0, 'A') }, d => { d.text.set(0, 'B') }]))
  return record('conflicts', 'concurrent assignments to one element: inside a typed run, on its last element, three at once, a number that wins', batches)
}

function mixedValues() {
  const a = new Peer(A)
  const batches = []
  batches.push([a.change(d => { d.text = new Automerge.Text('hello world') })])
  batches.push([a.change(d => { d.text.insertAt(2, { x: 3 }) })])
  batches.push([a.change(d => { d.text.insertAt(5, 42); d.text.insertAt(7, null); d.text.insertAt(9, true) })])
  batches.push([a.change(d => { d.text.insertAt(1, new Automerge.Counter(4)); d.text.insertAt(0, 2.5) })])
  batches.push([a.change(d => { d.text.insertAt(d.text.length, ...'!?') })])
  batches.push([a.change(d => { d.text.get(3).y = 'inside' })])
  return record('mixed_values', 'a Text that holds a number, null, true, a float, a nested map and a counter between its characters', batches)
}

function bom() {
  const a = new Peer(A)
  const batches = []
  batches.push([a.change(d => { d.text = new Automerge.Text('ab') })])
  batches.push([a.change(d => { d.text.insertAt(1, '\uFEFF') })])                  // an element that is U+FEFF alone
  batches.push([a.change(d => { d.text.insertAt(0, '\uFEFFab') })])                // a value that begins with it
  batches.push([a.change(d => { d.text.insertAt(4, 'x', '\uFEFF', '€', '\uFEFF', 'y') })])   // inside a run of three-byte values
  batches.push([a.change(d => { d.text.insertAt(2, 'q\uFEFF') })])                 // not at the start of its value: kept
  return record('bom', 'values that are, begin with, or hold U+FEFF: TextDecoder drops a leading one per value', batches)
}

function objects() {
  const a = new Peer(A)
  const setup = a.change(d => {
    d.title = new Automerge.Text('Title')
    d.list = [1, 'two', 3]
    d.meta = { body: new Automerge.Text('the body of the document'), n: 1 }
    d.empty = new Automerge.Text()
    d.gone = new Automerge.Text('to be deleted')
  })
  const b = new Peer(B, [setup])
  const batches = [[setup]]
  batches.push(round([a, b], [d => { d.gone.deleteAt(0, 13) }, d => { d.meta.body.insertAt(4, ...'whole ') }]))
  batches.push(round([a, b], [d => { d.fresh = new Automerge.Text(); d.fresh.insertAt(0, ...'made and typed into at once') }, d => { d.list.push('four') }]))
  batches.push(round([a, b], [d => { d.title.insertAt(5, ...' page') }, d => { d.fresh.insertAt(4, '—') }]))
  return record('objects', 'two Texts, a list and a map in one document; an empty Text; a Text whose characters are all deleted; a Text made and typed into in one change', batches)
}

// op ids of the counters a change makes inside lists, in op order
function counterIds(c) {
  const d = decodeChange(c), out = []
  let ctr = d.startOp
  for (const op of d.ops) {
    const n = op.values ? op.values.length : 1
    if (op.datatype === 'counter' && op.elemId) for (let k = 0; k < n; k++) out.push(`${ctr + k}@${d.actor}`)
    ctr += n
  }
  return out
}

function quirk() {
  // the frontend has no way to increment a counter that sits inside a Text: the increments and the deletion are encoded by hand
  const a = new Peer(A)
  const setup = a.change(d => { d.text = new Automerge.Text('count: '); d.text.insertAt(7, new Automerge.Counter(1)); d.text.insertAt(8, ...' and ', new Automerge.Counter(10), '.') })
  const s = decodeChange(setup), text = `1@${A}`, [first, second] = counterIds(setup)
  if (!first || !second) throw new Error('no two counters in the setup change')
  let maxOp = s.startOp + rowsOf(setup) - 1
  const seq = {}
  const hand = (actor, deps, ops) => {
    seq[actor] = (seq[actor] || 0) + 1
    const c = encodeChange({ actor, seq: seq[actor], startOp: maxOp + 1, time: 0, message: '', deps, ops })
    maxOp += ops.length
    return c
  }
  const batches = [[setup]]
  const inc1 = hand(B, [s.hash], [{ action: 'inc', obj: text, elemId: first, value: 2, pred: [first] }])
  const inc2 = hand(B, [decodeChange(inc1).hash], [{ action: 'inc', obj: text, elemId: first, value: 3, pred: [first] }])
  batches.push([inc1], [inc2])
  // the second counter deleted by one author while the other increments it: the deletion delivered first
  const del = hand(C, [decodeChange(inc2).hash], [{ action: 'del', obj: text, elemId: second, pred: [second] }])
  const inc3 = hand(B, [decodeChange(inc2).hash], [{ action: 'inc', obj: text, elemId: second, value: 5, pred: [second] }])
  batches.push([del], [inc3])
  const tail = hand(B, [decodeChange(del).hash, decodeChange(inc3).hash].sort(), [{ action: 'set', obj: text, elemId: '_head', insert: true, value: '>', pred: [] }])
  batches.push([tail])
  return record('quirk', 'a counter inside a Text incremented twice; another one deleted while the other author increments it (hand-encoded increments)', batches)
}

let sessions = []
for (const make of [typed, conflicts, mixedValues, bom, objects, quirk]) {
  try { sessions.push(make()) } catch (e) { console.log(make.name, 'dropped: the reference rejects it:', e.message) }
}
const file = path.join(ROOT, 'tests', 'golden', 'text', 'text_reads.json')
fs.mkdirSync(path.dirname(file), { recursive: true })
const write = () => fs.writeFileSync(file, JSON.stringify({ note: 'tools/fixtures/make_text_reads.js: reference frontend sessions and the string of every Text after every call', sessions }))
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
for (const s of sessions) console.log(s.name, s.batches.length, 'calls, rows', s.rows.join(' '), '|', s.texts[s.texts.length - 1].map(t => t.objectId.slice(0, 6) + ':' + t.length).join(' '))
console.log(file, fs.statSync(file).size, 'bytes')
