// TEST INFRASTRUCTURE (build container only: it needs the live reference): the sessions of tests/test_local_change.py and
// tests/test_js_local_change.py -- Backend.applyLocalChange call by call, the change REQUESTS made by the reference FRONTEND
// (Automerge.change on a document whose backend is a stub that records the request before passing it on to the reference's backend).
// Writes tests/golden/local/sessions.json: per session the calls
//   { kind: 'load', doc }                      Backend.load(doc) (base64); only as the first call
//   { kind: 'remote', batch, patch }           Backend.applyChanges(state, batch) (changes in base64), JSON.stringify(patch)
//   { kind: 'local', request, change, hash, patch }   Backend.applyLocalChange(state, request): binaryChange (base64), its hash, the patch
//   { kind: 'rejected', request, error }       a request the reference throws on, with the text of its exception; the state stays
// and at the end the whole-document patch and the SHA-256 of Backend.save. A session that starts with a load also holds the hashes of
// the document's changes (doc_hashes) and whether the reference had rebuilt the document's hash graph before its first applyChanges
// (graph_rebuilt): what tests/oracle_lib.py OracleSession needs to follow it.
// Data only. Then replays every session through the sequential oracle (OracleSession.apply(..., local=True)) and drops what it
// cannot follow.
//   NODE_PATH=oracle/js_shims/node_modules node tools/fixtures/make_local_change_sessions.js
const path = require('path')
const fs = require('fs')
const crypto = require('crypto')
const { spawnSync } = require('child_process')
const ROOT = path.join(__dirname, '..', '..')
const { loadBackend } = require(path.join(ROOT, 'oracle', 'js', 'ref_loader'))
const ref = loadBackend()
const { Backend, columnar } = ref
const Automerge = ref.Automerge()
const { decodeChange } = columnar
const id = d => d.repeat(32 / d.length)
const b64 = u8 => Buffer.from(u8.buffer, u8.byteOffset, u8.byteLength).toString('base64')
const copy = x => JSON.parse(JSON.stringify(x))

// The recorded replica: every call its document makes on the backend lands in `calls`
class Rec {
  constructor(actor, loadFrom) {
    this.calls = []
    const self = this
    this.backend = Object.assign({}, Backend, {
      applyLocalChange(state, request) {
        const asked = copy(request)   // (applyLocalChange rewrites request.deps)
        const r = Backend.applyLocalChange(state, request)
        self.calls.push({ kind: 'local', request: asked, change: b64(r[2]), hash: decodeChange(r[2]).hash, patch: JSON.stringify(r[1]) })
        self.last = r[2]
        return r
      },
      load(bytes) {
        self.calls.push({ kind: 'load', doc: b64(bytes) })
        return Backend.load(bytes)
      }
    })
    if (loadFrom) {
      const state = this.backend.load(loadFrom)
      this.doc = Automerge.Frontend.applyPatch(Automerge.init({ actorId: actor, backend: this.backend }), Backend.getPatch(state), state)
    } else this.doc = Automerge.init({ actorId: actor, backend: this.backend })
  }
  local(fn, options = {}) {
    this.doc = Automerge.change(this.doc, Object.assign({ time: 0 }, options), fn)
    return this.last
  }
  remote(batch) {
    const old = Automerge.Frontend.getBackendState(this.doc, 'applyChanges')
    const [state, patch] = Backend.applyChanges(old, batch)
    this.calls.push({ kind: 'remote', batch: batch.map(b64), patch: JSON.stringify(patch) })
    this.doc = Automerge.Frontend.applyPatch(this.doc, patch, state)
  }
  // a hand-made request the reference must throw on
  rejected(request) {
    const state = Automerge.Frontend.getBackendState(this.doc, 'applyLocalChange')
    let error = null
    try { Backend.applyLocalChange(state, copy(request)) } catch (e) { error = e.message }
    if (error === null) throw new Error('the reference accepted a request it was to reject')
    this.calls.push({ kind: 'rejected', request, error })
  }
  state() { return Automerge.Frontend.getBackendState(this.doc, 'save') }
}

// an ordinary replica that makes the remote changes
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

function finish(name, note, rec, extra = {}) {
  const state = rec.state()
  const whole_patch = JSON.stringify(Backend.getPatch(state))
  const save_sha256 = crypto.createHash('sha256').update(Backend.save(state)).digest('hex')
  return Object.assign({ name, note, calls: rec.calls, whole_patch, save_sha256 }, extra)
}

const A = id('7'), B = id('9'), C = id('b'), LAST = id('f'), FIRST = id('1')
const chars = (n, from = 0) => Array.from({ length: n }, (_, k) => String.fromCharCode(97 + (from + k) % 26))

function oneOp() {
  const r = new Rec(A)
  r.local(d => { d.x = 1 })
  r.local(d => { d.y = 'two' }, { message: 'the second change' })
  return finish('one_op', 'one set on a root key; the same author again: seq 2 depends on the last hash, with a message', r)
}

function textRuns() {
  const r = new Rec(A)
  const all = []
  const keep = c => { all.push(c); return c }
  keep(r.local(d => { d.text = new Automerge.Text() }))
  keep(r.local(d => { d.text.insertAt(0, 'h') }))                       // a head insert, run of 1
  keep(r.local(d => { d.text.insertAt(1, ...chars(2)) }))               // 2
  keep(r.local(d => { d.text.insertAt(0, ...chars(64, 3)) }))           // 64, at the head
  keep(r.local(d => { d.text.insertAt(10, ...chars(65, 5)) }))          // 65
  const b = new Peer(B, all)
  const cb = b.change(d => { d.text.insertAt(5, 'B', 'B', 'B') })
  r.remote([cb])
  r.local(d => { d.text.insertAt(7, 'x') })                             // behind an element of the other actor
  r.local(d => { d.text.insertAt(8, ...chars(5, 1)) })
  r.local(d => { d.text.insertAt(40, 'p'); d.text.insertAt(2, 'q') })   // element counters that go DOWN between rows: a negative keyCtr delta
  return finish('text_runs', 'multi-inserts into a Text: runs of 1, 2, 64, 65, at the head, behind an element of another actor, and two ' +
    'single inserts whose element counters descend', r)
}

function deletes() {
  const r = new Rec(A)
  r.local(d => { d.text = new Automerge.Text(chars(200).join('')) })
  r.local(d => { d.text.deleteAt(3, 2) })      // multiOp 2
  r.local(d => { d.text.deleteAt(20, 65) })    // multiOp 65
  r.local(d => { d.text.deleteAt(0) })         // a plain delete
  return finish('deletes', 'multiOp deletions of 2 and 65 elements and a single one', r)
}

function mixed() {
  const r = new Rec(A)
  r.local(d => { d.text = new Automerge.Text('0123456789'); d.cnt = new Automerge.Counter(1) })
  r.local(d => {
    d.text.insertAt(4, 'x', 'y', 'z')
    d.text.deleteAt(0, 2)
    d.key = 'v'
    d.m = { a: 1, b: 2 }
    d.cnt.increment(3)
  })
  return finish('mixed', 'one change of a 3-value insert, a multiOp 2 deletion, a key set, a makeMap with two sets inside, an inc: the row bases matter', r)
}

function predOrder() {
  // the author's id sorts last; its own value and one of another actor conflict on a key at EQUAL counters, then two other actors' do
  const r = new Rec(LAST)
  const c0 = r.local(d => { d.seed = 0 })
  const b = new Peer(B, [c0]), c = new Peer(C, [c0])
  const mine = r.local(d => { d.k = 'mine' })
  const cb = b.change(d => { d.k = 'b'; d.j = 'b' }), cc = c.change(d => { d.j = 'c' })   // k: 2@LAST and 2@B; j: 3@B and 2@C ...
  r.remote([cb])
  r.remote([cc])
  r.local(d => { d.k = 'both' })      // preds 2@B and 2@LAST: by id B first, by change-local number the author (0) first
  const c2 = c.change(d => { d.i = 'c' })
  const b2 = new Peer(FIRST, [c0]).change(d => { d.j2 = 0; d.i = '1' })
  r.remote([c2, b2])
  r.local(d => { d.i = 'all'; d.j = 'all' })
  void mine
  return finish('pred_order', 'ops with two preds of equal counter: the author (whose id sorts last, local number 0) and another actor; two other actors', r)
}

function numbers() {
  const r = new Rec(A)
  r.local(d => {
    d.n63 = 63; d.n64 = 64; d.m64 = -64; d.m65 = -65; d.p31 = 2 ** 31; d.max = 2 ** 53 - 1; d.min = -(2 ** 53 - 1)
    d.u = new Automerge.Uint(300); d.c = new Automerge.Counter(10); d.t = new Date(1234567890123)
    d.f = 1.5; d.fi = new Automerge.Float64(3); d.i = new Automerge.Int(-7)
    d.empty = ''; d.utf = 'héllo € 𝄞'; d.nul = null; d.yes = true; d.no = false
    d.list = [1, 2, 3, 'a', 'b', null, true, 1.5, 2.5]
  })
  return finish('numbers', 'values at the LEB128 length boundaries, every datatype, strings of 0 bytes and of multi-byte characters, null / true / false', r)
}

function withDeps() {
  const r = new Rec(A)
  r.local(d => { d.a = 1 })
  const b = new Peer(B)
  const cb = b.change(d => { d.b = 1 })   // concurrent: does not know the author's change
  r.remote([cb])
  r.local(d => { d.a = 2 })               // deps: the other's head and the own last hash, sorted
  r.local(d => { d.a = 3 })
  return finish('deps', 'a remote change of a second actor, then local changes: the deps are the other head plus the own last hash', r)
}

// two sessions whose last change straddles DEFLATE_MIN_SIZE = 256 bytes
function deflatePair() {
  const sizeOf = n => { const r = new Rec(A); r.local(d => { d.text = new Automerge.Text() }); return [r, r.local(d => { d.text.insertAt(0, ...chars(n).map((c, k) => c + (k % 7))) })] }
  let n = 1
  while (sizeOf(n)[1][8] === 1) n++
  const [below] = sizeOf(n - 1), [above] = sizeOf(n)
  return [finish('deflate_below', `an insert of ${n - 1} two-byte values: the largest change that stays uncompressed (byte 8 is 1)`, below),
    finish('deflate_above', `an insert of ${n} two-byte values: the smallest change that is DEFLATEd (byte 8 is 2)`, above)]
}

function docOf() {
  const a = new Peer(A)
  const cs = [a.change(d => { d.text = new Automerge.Text('loaded'); d.n = 1 }), a.change(d => { d.n = 2 })]
  const b = new Peer(B, cs)
  cs.push(b.change(d => { d.text.insertAt(3, '-') }))
  a.see([cs[2]])
  const doc = Automerge.save(a.doc)
  const hashes = Backend.getAllChanges(Backend.load(doc)).map(c => decodeChange(c).hash)
  return { doc, doc_hashes: hashes.join('') }
}

function loadedNewActor() {
  const { doc, doc_hashes } = docOf()
  const r = new Rec(C, doc)
  r.local(d => { d.text.insertAt(0, 'n', 'e', 'w') })
  r.local(d => { d.n = 3 })
  return finish('loaded_new_actor', 'Backend.load, then two local changes of an actor new to the document: the hash graph is never rebuilt', r, { doc_hashes, graph_rebuilt: false })
}

function loadedOwnAuthor() {
  const { doc, doc_hashes } = docOf()
  const r = new Rec(A, doc)
  r.local(d => { d.text.insertAt(6, '!') })   // seq 3: the hash of seq 2 lies inside the document: the reference rebuilds the hash graph first
  r.local(d => { d.n = 4 })
  return finish('loaded_own_author', "Backend.load, then local changes of the document's own author (seq > 1): the reference rebuilds the hash graph before the first", r,
    { doc_hashes, graph_rebuilt: true })
}

function rejects() {
  const r = new Rec(A)
  r.local(d => { d.text = new Automerge.Text('ab') })
  const first = copy(r.calls[0].request)
  r.rejected(first)   // seq 1 again
  r.rejected({ actor: A, seq: 2, startOp: 4, time: 0, message: '', deps: [],
    ops: [{ action: 'set', obj: `1@${A}`, elemId: `3@${A}`, insert: true, values: ['x', 'y'], pred: [`3@${A}`] }] })
  r.rejected({ actor: A, seq: 2, startOp: 4, time: 0, message: '', deps: [],
    ops: [{ action: 'set', obj: `1@${A}`, elemId: `3@${A}`, insert: true, values: ['x', 7], pred: [] }] })
  r.local(d => { d.text.insertAt(2, 'c') })   // the state is as it was
  return finish('rejected', 'a seq already applied, a multi-insert with a pred, a multi-insert with a bad value / datatype pair; then a good change', r)
}

let sessions = []
for (const make of [oneOp, textRuns, deletes, mixed, predOrder, numbers, withDeps, deflatePair, loadedNewActor, loadedOwnAuthor, rejects]) {
  try { sessions = sessions.concat(make()) } catch (e) { console.log(make.name, 'dropped: the reference rejects it:', e.message) }
}
const dir = path.join(ROOT, 'tests', 'golden', 'local')
fs.mkdirSync(dir, { recursive: true })
const file = path.join(dir, 'sessions.json')
const write = () => fs.writeFileSync(file, JSON.stringify({ note: 'tools/fixtures/make_local_change_sessions.js: Backend.applyLocalChange sessions, the requests made by the reference frontend', sessions }))
write()

// the sequential oracle against the file just written: one line per session, `name ok` or `name FAILS ...`
const check = `
import sys
sys.path.insert(0, ${JSON.stringify(path.join(ROOT, 'tests'))}); sys.path.insert(0, ${JSON.stringify(ROOT)})
import json
import test_local_change as t
for s in json.load(open(${JSON.stringify(file)}))["sessions"]:
    bad = None
    try:
        t.check_session_against_oracle(s)
    except Exception as e:
        bad = repr(e)[:300].replace("\\n", " ")
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
for (const s of sessions) console.log(s.name, s.calls.map(c => c.kind).join(' '))
console.log(file, fs.statSync(file).size, 'bytes')
