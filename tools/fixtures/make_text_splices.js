// TEST INFRASTRUCTURE (build container only: it needs the live reference): the sessions of tests/test_text_splice.py and
// js/test_text_splice.js -- a Text edited by POSITION. The reference FRONTEND + the reference BACKEND execute
// Automerge.change(doc, {time}, d => d.text.deleteAt(i, n) / d.text.insertAt(i, ...chars)); the backend of the recorded replica is a stub
// that records the change REQUEST the frontend hands to applyLocalChange before passing it on.
// Writes tests/golden/text/text_splices.json: per session `changes` (every binary change of the session in the order it was applied,
// base64) and `calls`, each with n_before = how many of `changes` were applied before it:
//   { kind: 'apply', n }            the next n changes arrive through Backend.applyChanges (the setup, other actors' typing)
//   { kind: 'splice', objectId, start, deletions, values, actor, time, request, change, patch, text }
//                                   one context.splice: the request the frontend produced, the binary change, the patch applyLocalChange
//                                   returned (JSON text) and the Text's string afterwards. request / change / patch are null where the
//                                   frontend made no change (nothing deleted, nothing inserted)
//   { kind: 'counter', ...as 'splice' }   a deletion that reaches a Counter, executed on a COPY of the replica (the session goes on without
//                                   it): context.js:455-471 throws a TypeError for a counter in a LIST, but it looks the element up as
//                                   object[index], which a Text does not have -- for a Text the frontend does not throw and deletes the
//                                   counter. Recorded as the reference did it; the engine refuses such a call (include/am355.h)
//   { kind: 'throws', objectId, start, deletions, values, actor, time, error, message }
//                                   a call the frontend throws on: the class and text of its exception; the state stays
// A call that deletes AND inserts is recorded from d.text.deleteAt(i, n) followed by d.text.insertAt(i, ...) in one change: two
// context.splice calls whose ops are those of one splice(i, n, values) -- the insertion's reference element, i - 1, is not among the deleted.
// Data only.
//   NODE_PATH=oracle/js_shims/node_modules node tools/fixtures/make_text_splices.js
const path = require('path')
const fs = require('fs')
const ROOT = path.join(__dirname, '..', '..')
const { loadBackend } = require(path.join(ROOT, 'oracle', 'js', 'ref_loader'))
const ref = loadBackend()
const { Backend, columnar } = ref
const Automerge = ref.Automerge()
const { decodeChange, encodeChange } = columnar
const id = d => d.repeat(32 / d.length)
const b64 = u8 => Buffer.from(u8.buffer, u8.byteOffset, u8.byteLength).toString('base64')
const copy = x => JSON.parse(JSON.stringify(x))

// The recorded replica: its frontend document sits on the reference backend through a stub that keeps the last request
class Rec {
  constructor(actor) {
    this.actor = actor
    this.changes = []
    this.calls = []
    this.clock = 0
    const self = this
    this.backend = Object.assign({}, Backend, {
      applyLocalChange(state, request) {
        const asked = copy(request)   // (applyLocalChange rewrites request.deps)
        const r = Backend.applyLocalChange(state, request)
        self.last = { request: asked, change: r[2], patch: JSON.stringify(r[1]) }
        return r
      }
    })
    this.doc = Automerge.init({ actorId: actor, backend: this.backend })
  }
  get objectId() { return Automerge.getObjectId(this.doc.text) }
  // changes of other replicas (or the setup) through Backend.applyChanges
  apply(batch) {
    const old = Automerge.Frontend.getBackendState(this.doc, 'applyChanges')
    const [state, patch] = Backend.applyChanges(old, batch)
    this.calls.push({ kind: 'apply', n: batch.length, n_before: this.changes.length })
    this.changes.push(...batch)
    this.doc = Automerge.Frontend.applyPatch(this.doc, patch, state)
  }
  // a change of this replica that is no splice (the setup): recorded as an applied change
  setup(fn) {
    this.doc = Automerge.change(this.doc, { time: 0 }, fn)
    this.calls.push({ kind: 'apply', n: 1, n_before: this.changes.length })
    this.changes.push(this.last.change)
    return this.last.change
  }
  splice(start, deletions, values = []) {
    const time = ++this.clock
    const call = { objectId: this.objectId, start, deletions, values, actor: this.actor, time, n_before: this.changes.length }
    this.last = null
    try {
      this.doc = Automerge.change(this.doc, { time }, d => {
        if (deletions > 0 || values.length === 0) d.text.deleteAt(start, deletions)
        if (values.length > 0) d.text.insertAt(start, ...values)
      })
    } catch (e) {
      if (!(e instanceof RangeError) && !(e instanceof TypeError)) throw e
      this.calls.push(Object.assign(call, { kind: 'throws', error: e instanceof RangeError ? 'RangeError' : 'TypeError', message: e.message }))
      return null
    }
    const made = this.last
    this.calls.push(Object.assign(call, { kind: 'splice', request: made && made.request, change: made && b64(made.change), patch: made && made.patch,
      text: this.doc.text.toString(), length: this.doc.text.length }))
    if (made) this.changes.push(made.change)
    return made && made.change
  }
  // the same call on a copy of this replica: recorded under `kind`, the replica stays as it is
  probe(kind, start, deletions, values = []) {
    const copyOf = new Rec(this.actor)
    copyOf.apply(this.changes)
    copyOf.clock = this.clock
    copyOf.splice(start, deletions, values)
    const call = copyOf.calls[copyOf.calls.length - 1]
    if (call.kind !== 'splice' || !call.request) throw new Error('the probe made no change: ' + JSON.stringify(call))
    this.calls.push(Object.assign(call, { kind, n_before: this.changes.length }))
  }
  get length() { return this.doc.text.length }
}

// an ordinary replica that makes the other actors' changes
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

const finish = (name, note, rec) => ({ name, note, changes: rec.changes.map(b64), calls: rec.calls, whole_patch: JSON.stringify(Backend.getPatch(Automerge.Frontend.getBackendState(rec.doc, 'save'))) })
const A = id('3'), B = id('8'), C = id('d')

function typed() {
  const r = new Rec(A)
  r.setup(d => { d.text = new Automerge.Text() })
  r.splice(0, 0, [...'The quick brown fox'])          // a pasted run into the empty Text
  r.splice(19, 0, ['.'])                               // a keystroke at the end
  r.splice(4, 0, [...'very '])                         // a pasted run in the middle
  r.splice(9, 0, ['!'])
  r.splice(0, 0, ['>'])                                // at the head
  r.splice(3, 4)                                       // inside one run
  r.splice(2, 9)                                       // across runs
  r.splice(5, 1)                                       // a single element
  r.splice(6, 0, [...'jumps over'])
  r.splice(1, 3, [...'xyz'])                           // 3 deleted + 3 inserted
  r.splice(r.length - 2, 2, ['é', '€'])
  for (let k = 0; k < 6; k++) r.splice((5 * k + 3) % r.length, 0, [String.fromCharCode(65 + k)])
  r.splice(2, 12)
  r.splice(r.length, 0, [...' the end'])
  return finish('typed', 'one actor: pasted runs, single characters, deletions inside one run, across runs, of single elements, deletions with insertions', r)
}

function twoActors() {
  const a = new Peer(A)
  const all = [a.change(d => { d.text = new Automerge.Text() })]
  const b = new Peer(B, all)
  // character by character, turn by turn: neighbouring elements have different actors
  for (let k = 0; k < 12; k++) {
    const p = k % 2 ? b : a, q = k % 2 ? a : b
    const c = p.change(d => { d.text.insertAt(d.text.length, String.fromCharCode(97 + k)) })
    q.see([c])
    all.push(c)
  }
  const r = new Rec(C)
  r.apply(all)
  r.splice(2, 5)                                       // five deletions, five ops
  r.splice(1, 0, [...'XY'])
  r.splice(0, 3)                                       // the other actor's element, then this replica's own run
  r.splice(2, 2, ['m'])
  const more = [a.change(d => { d.text.insertAt(1, 'q') })]   // concurrent with the replica's edits
  r.apply(more)
  r.splice(0, r.length - 1)
  r.splice(1, 0, [...'again'])
  return finish('two_actors', 'two actors typing character by character in turns, merged: every deletion is an op of its own; a third actor edits by position', r)
}

function conflicts() {
  const a = new Peer(A)
  const setup = a.change(d => { d.text = new Automerge.Text('abcdefghij') })
  const b = new Peer(B, [setup])
  const ca = a.change(d => { d.text.set(4, 'X') }), cb = b.change(d => { d.text.set(4, 'Y') })
  a.see([cb]); b.see([ca])
  const ca2 = a.change(d => { d.text.set(9, '1') }), cb2 = b.change(d => { d.text.set(9, '2') })   // on the last element of the run
  a.see([cb2]); b.see([ca2])
  const ca3 = a.change(d => { d.text.set(0, 'A') })                                                  // an assignment without a conflict
  b.see([ca3])
  const r = new Rec(C)
  r.apply([setup])
  r.apply([ca, cb])
  r.apply([ca2, cb2, ca3])
  r.splice(5, 0, ['+'])          // behind the conflicting element: it is the reference element
  r.splice(4, 0, ['-'])          // before it
  r.splice(5, 1)                 // the conflicting element itself: the pred is the last update's
  r.splice(2, 4)                 // a range over where it was
  r.splice(r.length - 1, 1)      // the conflicting last element
  r.splice(0, 2, [...'zz'])      // the assigned first element and its neighbour
  r.splice(r.length, 0, ['$'])
  return finish('conflicts', 'concurrent text.set(i, v) of two actors merged, then deletions and insertions at, before and behind the conflicting index', r)
}

function holes() {
  const r = new Rec(A)
  r.setup(d => { d.text = new Automerge.Text() })
  r.splice(0, 0, [...'0123456789abcdefghijklmnopqrstuvwxyz'])
  r.splice(10, 3)                // a counter gap inside the run
  r.splice(20, 1)
  r.splice(5, 20)                // over both gaps: the runs split there
  r.splice(3, 0, [...'NEW'])     // elements with later counters in the middle
  r.splice(0, r.length - 1)      // old run, new run, old run
  r.splice(0, 1, [...'fresh'])
  return finish('holes', 'deletions that leave counter gaps inside a pasted run: later deletions over the gaps split into several ops', r)
}

function edges() {
  const r = new Rec(A)
  r.setup(d => { d.text = new Automerge.Text() })
  r.splice(0, 0)                       // nothing deleted, nothing inserted, an empty Text: no change
  r.splice(0, 1)                       // out of bounds on the empty Text
  r.splice(0, 0, ['a'])                // one value: a plain inserting set at _head
  r.splice(1, 0, ['b', 'c'])           // several: `values`; start == length
  r.splice(0, 0, ['é', '€', '😀'])     // 2, 3 and 4 bytes (an astral character) at _head
  r.splice(3, 0)                       // deletions == 0, no insertions: no change
  r.splice(6, 0, ['z'])                // start == length
  r.splice(7, 1)                       // start == length, one deletion: out of bounds
  r.splice(8, 0, ['y'])                // start > length
  r.splice(3, 5)                       // start + deletions > length
  r.splice(2, 1, ['🌍'])
  r.splice(0, r.length)                // the whole text
  r.splice(0, 0, [...'back'])          // into the emptied Text: _head again
  r.splice(0, r.length, ['x'])         // everything replaced
  return finish('edges', 'start 0, start == length, the whole text deleted, one inserted value against several, multi-byte and astral characters, nothing to do, out of bounds', r)
}

function counters() {
  // a counter inside a Text; the frontend cannot increment it: the increment is encoded by hand (the approach of text_reads.json)
  const a = new Peer(A)
  const setup = a.change(d => { d.text = new Automerge.Text('ab'); d.text.insertAt(1, new Automerge.Counter(3)); d.text.insertAt(3, 'c', new Automerge.Counter(7), 'd') })
  const s = decodeChange(setup)
  const ids = []
  let ctr = s.startOp
  for (const op of s.ops) {
    const n = op.values ? op.values.length : 1
    if (op.datatype === 'counter' && op.elemId) for (let k = 0; k < n; k++) ids.push(`${ctr + k}@${s.actor}`)
    ctr += n
  }
  if (ids.length !== 2) throw new Error('no two counters in the setup change')
  const inc = encodeChange({ actor: B, seq: 1, startOp: ctr, time: 0, message: '', deps: [s.hash],
    ops: [{ action: 'inc', obj: `1@${A}`, elemId: ids[1], value: 5, pred: [ids[1]] }] })
  const r = new Rec(C)
  r.apply([setup])                     // a C3 b c C7 d
  r.probe('counter', 1, 1)             // the counter nobody incremented
  r.probe('counter', 0, 3)             // a range that holds it
  r.splice(2, 0, ['+'])                // behind it: the counter is the reference element only      a C3 + b c C7 d
  r.apply([inc])
  r.probe('counter', 5, 1)             // the incremented counter
  r.probe('counter', 4, 3, ['x'])
  r.splice(0, 1)                       // beside the counters: fine                                  C3 + b c C7 d
  r.splice(5, 1, ['e'])                // behind the incremented counter: it is the reference element
  r.splice(1, 3)                       // between the counters
  return finish('counters', 'counters inside a Text, one incremented by a hand-encoded change: what the reference does when a deletion reaches them, and edits around them', r)
}

const sessions = [typed(), twoActors(), conflicts(), holes(), edges(), counters()]
const file = path.join(ROOT, 'tests', 'golden', 'text', 'text_splices.json')
fs.mkdirSync(path.dirname(file), { recursive: true })
fs.writeFileSync(file, JSON.stringify({ note: 'tools/fixtures/make_text_splices.js: reference frontend + backend sessions of text.deleteAt / text.insertAt, with the change requests the frontend produced', sessions }))
for (const s of sessions) console.log(s.name, s.calls.map(c => (c.kind === 'apply' ? 'apply' + c.n : c.kind === 'throws' ? c.error : (c.kind === 'counter' ? 'counter:' : '') + (c.request ? c.request.ops.length + 'op' : 'nothing'))).join(' '))
console.log(file, fs.statSync(file).size, 'bytes')
