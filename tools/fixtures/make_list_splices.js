// TEST INFRASTRUCTURE (build container only: it needs the live reference): the sessions of tests/test_list_splice.py and
// js/test_list_splice.js -- a plain LIST edited by POSITION. The reference FRONTEND + the reference BACKEND execute
// Automerge.change(doc, {time}, d => d.list.deleteAt(i, n) / d.list.insertAt(i, ...values) / d.list[i] = v); the backend of the recorded
// replica is a stub that records the change REQUEST the frontend hands to applyLocalChange before passing it on.
// Writes tests/golden/list/list_splices.json: per session `changes` (every binary change of the session in the order it was applied,
// base64) and `calls`, each with n_before = how many of `changes` were applied before it:
//   { kind: 'apply', n }            the next n changes arrive through Backend.applyChanges (the setup, other actors' edits)
//   { kind: 'splice', objectId, start, deletions, values, actor, time, request, change, patch, list, length }
//                                   one context.splice: the request the frontend produced, the binary change, the patch applyLocalChange
//                                   returned (JSON text), the list afterwards (JSON text) and its length. request / change / patch are
//                                   null where the frontend made no change (nothing deleted, nothing inserted)
//   { kind: 'set', objectId, index, value, actor, time, request, change, patch, list, length }
//                                   one context.setListIndex (d.list[index] = value); only assignments the reference emits an op for
//   { kind: 'throws', call: 'splice' | 'set', ...its arguments, error, message }
//                                   a call the frontend throws on: the class and text of its exception; the state stays
// VALUES are written as [class, v] pairs, which JSON keeps apart: ['str', 'a'], ['bool', true], ['null', null], ['int', 1],
// ['float64', 2.5], ['uint', 7], ['timestamp', ms], ['counter', 3]. A plain JS number is 'int' when it is a safe integer, else 'float64'
// (frontend/context.js:83-88); Uint / Float64 / Date / Counter are made with their classes.
// A call that deletes nothing is d.list.insertAt(i, ...values), with no values too (list.deleteAt(i, 0) deletes one element).
// A call that deletes AND inserts is recorded from d.list.deleteAt(i, n) followed by d.list.insertAt(i, ...) in one change: two
// context.splice calls whose ops are those of one splice(i, n, values).
// Data only.
//   NODE_PATH=oracle/js_shims/node_modules node tools/fixtures/make_list_splices.js
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

// [class, v] -> the JS value the frontend is given
function js(pair) {
  const [cls, v] = pair
  switch (cls) {
    case 'str': case 'bool': case 'null': return v
    case 'int': return v
    case 'float64': return Number.isInteger(v) ? new Automerge.Float64(v) : v
    case 'uint': return new Automerge.Uint(v)
    case 'timestamp': return new Date(v)
    case 'counter': return new Automerge.Counter(v)
    default: throw new Error('value class ' + cls)
  }
}
const S = s => ['str', s], I = n => ['int', n]

// The recorded replica: its frontend document sits on the reference backend through a stub that keeps the last request
class Rec {
  constructor(actor, key = 'list') {
    this.actor = actor
    this.key = key
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
  get list() { return this.doc[this.key] }
  get objectId() { return Automerge.getObjectId(this.list) }
  get length() { return this.list.length }
  apply(batch) {
    const old = Automerge.Frontend.getBackendState(this.doc, 'applyChanges')
    const [state, patch] = Backend.applyChanges(old, batch)
    this.calls.push({ kind: 'apply', n: batch.length, n_before: this.changes.length })
    this.changes.push(...batch)
    this.doc = Automerge.Frontend.applyPatch(this.doc, patch, state)
  }
  setup(fn) {
    this.doc = Automerge.change(this.doc, { time: 0 }, fn)
    this.calls.push({ kind: 'apply', n: 1, n_before: this.changes.length })
    this.changes.push(this.last.change)
    return this.last.change
  }
  run(kind, call, fn) {
    const time = ++this.clock
    Object.assign(call, { objectId: this.objectId, actor: this.actor, time, n_before: this.changes.length })
    this.last = null
    try {
      this.doc = Automerge.change(this.doc, { time }, fn)
    } catch (e) {
      if (!(e instanceof RangeError) && !(e instanceof TypeError)) throw e
      this.calls.push(Object.assign({ kind: 'throws', call: kind }, call, { error: e instanceof RangeError ? 'RangeError' : 'TypeError', message: e.message }))
      return null
    }
    const made = this.last
    this.calls.push(Object.assign({ kind }, call, { request: made && made.request, change: made && b64(made.change), patch: made && made.patch,
      list: JSON.stringify(this.list), length: this.list.length }))
    if (made) this.changes.push(made.change)
    return made && made.change
  }
  splice(start, deletions, values = []) {
    const k = this.key
    return this.run('splice', { start, deletions, values }, d => {
      if (deletions > 0) d[k].deleteAt(start, deletions)   // (list.deleteAt(i, 0) deletes ONE element: numDelete || 1)
      if (values.length > 0 || deletions === 0) d[k].insertAt(start, ...values.map(js))
    })
  }
  set(index, value) {
    const k = this.key
    const made = this.run('set', { index, value }, d => { d[k][index] = js(value) })
    const call = this.calls[this.calls.length - 1]
    if (call.kind === 'set' && !call.request) throw new Error('an assignment the reference emits no op for: not recorded, choose another value')
    return made
  }
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
const A = id('3'), B = id('8'), C = id('d'), D = id('5')

function typed() {
  const r = new Rec(A)
  r.setup(d => { d.list = [] })
  r.splice(0, 0, [1, 2, 3, 4, 5, 6, 7, 8].map(I))       // a multi-insert of ints into the empty list
  r.splice(8, 0, [I(9)])                                 // one value at the end
  r.splice(4, 0, [40, 41, 42].map(I))                    // a multi-insert in the middle
  r.splice(0, 0, [I(0)])                                 // at the head
  r.splice(3, 4)                                         // inside and across runs
  r.splice(2, 1)                                         // a single element
  r.set(1, I(100))                                       // an assignment without a conflict
  r.set(1, I(101))                                       // onto the assigned element: the pred is the update's
  r.splice(0, 3)                                         // a range over the assigned element
  r.splice(1, 2, [70, 71].map(I))                        // 2 deleted + 2 inserted
  for (let k = 0; k < 4; k++) r.splice((3 * k + 1) % r.length, 0, [I(200 + k)])
  r.splice(1, r.length - 2)
  r.splice(r.length, 0, [300, 301, 302].map(I))
  return finish('typed', 'one actor: multi-inserts of ints, single values, deletions inside one run, across runs, assignments and deletions over them', r)
}

function mixedValues() {
  const r = new Rec(A)
  r.setup(d => { d.list = [] })
  r.splice(0, 0, [S('a'), ['bool', true], ['null', null]])      // no datatype on any: one multi-insert
  r.splice(1, 0, [I(1), ['float64', 2.5]])                       // int and float64: two sets
  r.splice(0, 0, [I(1), S('a')])                                 // int and none: two sets
  r.splice(2, 0, [['timestamp', 1600000000000]])                 // a Date
  r.splice(2, 0, [['timestamp', 1600000000000], ['timestamp', 1600000000001]])   // two Dates: one multi-insert with datatype
  r.splice(r.length, 0, [['uint', 7], ['uint', 8]])
  r.splice(0, 0, [['float64', 3], ['float64', 4.5]])             // Float64(3) and a plain 4.5: both float64
  r.splice(3, 0, [['counter', 10]])                              // a Counter inserted
  r.splice(r.length, 0, [['counter', 1], ['counter', 2]])        // two Counters
  r.splice(1, 0, [S('é€😀'), S('')])
  r.splice(0, 0, [['bool', false], ['null', null], S('x'), I(-5)])   // the last one breaks the class: four sets
  r.set(0, ['float64', 1.25])
  r.set(1, ['timestamp', 5])
  r.set(2, ['uint', 9])
  r.set(4, ['null', null])
  r.set(5, ['bool', true])
  return finish('mixed_values', 'values of every class: insertions that are one multi-insert and insertions that are one set per value; assignments of every class', r)
}

function twoActors() {
  const a = new Peer(A)
  const all = [a.change(d => { d.list = [] })]
  const b = new Peer(B, all)
  for (let k = 0; k < 10; k++) {   // element by element, turn by turn: neighbouring elements have different actors
    const p = k % 2 ? b : a, q = k % 2 ? a : b
    const c = p.change(d => { d.list.insertAt(d.list.length, k) })
    q.see([c])
    all.push(c)
  }
  const r = new Rec(C)
  r.apply(all)
  r.splice(2, 5)                                         // five deletions, five ops
  r.splice(1, 0, [S('X'), S('Y')])
  const c1 = a.change(d => { d.list.insertAt(1, 'q') })  // concurrent with the replica's edits
  r.apply([c1])
  r.splice(0, 3)
  r.set(2, S('m'))
  const c2 = b.change(d => { d.list.insertAt(0, 'r', 's') })
  r.apply([c2])
  r.splice(2, 2, [S('n')])
  r.splice(0, r.length - 1)
  r.splice(1, 0, [1, 2, 3].map(I))
  return finish('two_actors', 'two actors inserting element by element in turns, merged, and remote changes between the calls of a third actor that edits by position', r)
}

function conflicts() {
  const a = new Peer(A)
  const setup = a.change(d => { d.list = ['a', 'b', 'c', 'd', 'e', 'f', 'g', 'h', 'i', 'j'] })
  const b = new Peer(B, [setup]), e = new Peer(D, [setup])
  const ca = a.change(d => { d.list[4] = 'X' }), cb = b.change(d => { d.list[4] = 'Y' })               // two values
  const c7 = [a.change(d => { d.list[7] = 1 }), b.change(d => { d.list[7] = 2 }), e.change(d => { d.list[7] = 3 })]   // three values
  const c9 = [a.change(d => { d.list[9] = 'p' }), b.change(d => { d.list[9] = 'q' })]                  // on the last element of the record
  const c0 = [b.change(d => { d.list[0] = 'A' }), e.change(d => { d.list[0] = 'B' })]                  // on element 0
  const c2 = [a.change(d => { d.list[2] = 'solo' })]                                                    // an assignment without a conflict
  const r = new Rec(C)
  r.apply([setup])
  r.apply([ca, cb])
  r.apply([...c7, ...c9, ...c0, ...c2])
  r.splice(5, 0, [S('+')])       // behind a conflicted element: it is the reference element
  r.splice(4, 1)                 // the conflicted element: every value's id is a pred
  r.set(7, S('won'))             // an assignment onto three values: three preds (index 8 before the deletion: now 7)
  r.set(0, S('first'))           // onto the conflicted element 0
  r.splice(0, 3)                 // a range that begins at the (resolved) element 0 and crosses the assigned element 2
  r.splice(2, 5)                 // a range across the element of three values (resolved) up to the conflicted last one
  r.splice(r.length - 1, 1)
  r.splice(0, 0, [S('$')])
  // a fresh conflict of three actors, deleted within a range
  const now = r.changes.slice()
  const a2 = new Peer(A, now), b2 = new Peer(B, now), e2 = new Peer(D, now)
  r.apply([a2.change(d => { d.list[1] = 'u' }), b2.change(d => { d.list[1] = 'v' }), e2.change(d => { d.list[1] = 'w' })])
  r.splice(0, r.length)
  return finish('conflicts', 'two and three actors assign the same index concurrently; the index is then deleted, assigned, and deleted within ranges', r)
}

function holes() {
  const r = new Rec(A)
  r.setup(d => { d.list = [] })
  r.splice(0, 0, Array.from({ length: 36 }, (_, k) => I(k)))
  r.splice(10, 3)                // a counter gap inside the run
  r.splice(20, 1)
  r.splice(5, 20)                // over both gaps: the runs split there
  r.splice(3, 0, [S('N'), S('E'), S('W')])
  r.splice(0, r.length - 1)      // old run, new run, old run
  r.splice(0, 1, [1, 2, 3, 4, 5].map(I))
  return finish('holes', 'deletions that leave counter gaps (tombstones) inside a multi-insert: later deletions over the gaps split into several ops', r)
}

function children() {
  const a = new Peer(A)
  const all = [a.change(d => { d.cards = [] })]
  for (let k = 0; k < 6; k++) all.push(a.change(d => { d.cards.push({ title: 'card ' + k, done: k % 2 === 0 }) }))
  const b = new Peer(B, all)
  all.push(b.change(d => { d.cards.insertAt(2, { title: 'from b' }, { title: 'also b' }) }))
  const r = new Rec(C, 'cards')
  r.apply(all)
  r.splice(3, 1)                 // one card by position
  r.splice(0, 2)
  r.splice(1, 3)                 // across the two actors' cards
  r.splice(1, 0, [S('a plain value between cards')])
  r.set(0, S('replaced card'))   // an assignment onto a child object
  r.splice(0, r.length)
  return finish('children', 'a list of maps built through applyChanges; cards deleted by position, one replaced by a value', r)
}

function counters() {
  // the frontend cannot increment a counter that is not the shown value of its element: increments are encoded by hand
  const a = new Peer(A)
  const setup = a.change(d => { d.list = ['a', new Automerge.Counter(3), 'b', 'c', new Automerge.Counter(7), 'd', 'e'] })
  const s = decodeChange(setup)
  const ids = []
  let ctr = s.startOp
  for (const op of s.ops) {
    if (op.datatype === 'counter' && op.elemId) ids.push(`${ctr}@${s.actor}`)
    ctr += op.values ? op.values.length : 1
  }
  if (ids.length !== 2) throw new Error('no two counters in the setup change')
  const LIST = `1@${A}`
  const inc = encodeChange({ actor: B, seq: 1, startOp: ctr, time: 0, message: '', deps: [s.hash],
    ops: [{ action: 'inc', obj: LIST, elemId: ids[1], value: 5, pred: [ids[1]] }] })
  const r = new Rec(C)
  r.apply([setup])                       // a C3 b c C7 d e
  r.splice(1, 1)                         // TypeError: the counter nobody incremented
  r.splice(0, 3)                         // TypeError: a range that holds it
  r.set(1, S('x'))                       // RangeError: an assignment onto a counter
  r.splice(2, 0, [S('+')])               // behind it: the counter is the reference element only      a C3 + b c C7 d e
  r.apply([inc])
  r.splice(5, 1)                         // TypeError: the incremented counter
  r.splice(4, 3, [S('x')])               // TypeError
  r.set(5, I(0))                         // RangeError
  r.splice(0, 1)                         // beside the counters: fine                                  C3 + b c C7 d e
  r.splice(5, 1, [S('E')])               // behind the incremented counter: it is the reference element
  // a conflicted element of which one value is a counter completed by increments: D assigns a Counter to index 2 (`b`), the replica's
  // peer B assigns a string concurrently, then the counter is incremented (by hand: it may not be the shown value)
  const now = r.changes.slice()
  const dd = new Peer(D, now), bb = new Peer(B, now)
  const cd = dd.change(d => { d.list[2] = new Automerge.Counter(20) }), cbb = bb.change(d => { d.list[2] = 'text' })
  const dcd = decodeChange(cd)
  const inc2 = encodeChange({ actor: D, seq: dcd.seq + 1, startOp: dcd.startOp + 1, time: 0, message: '', deps: [dcd.hash],
    ops: [{ action: 'inc', obj: LIST, elemId: dcd.ops[0].elemId, value: 4, pred: [`${dcd.startOp}@${D}`] }] })
  r.apply([cd, cbb])
  r.apply([inc2])
  r.set(2, S('resolved'))                // RangeError: the incremented counter stands last among the values and is the one shown
  r.splice(1, 2)                         // TypeError
  // the same with the string assigned by a LATER op id than the increment: the string is shown, the counter is a hidden value
  const d3 = new Peer(D, r.changes.slice()), b3 = new Peer(B, r.changes.slice())
  const cd3 = d3.change(d => { d.list[3] = new Automerge.Counter(30) })
  b3.change(d => { d.pad = 1 })
  const pads = [Automerge.getLastLocalChange(b3.doc), b3.change(d => { d.pad = 2 }), b3.change(d => { d.pad = 3 })]
  const cb3 = b3.change(d => { d.list[3] = 'later' })
  const dcd3 = decodeChange(cd3)
  const inc3 = encodeChange({ actor: D, seq: dcd3.seq + 1, startOp: dcd3.startOp + 1, time: 0, message: '', deps: [dcd3.hash],
    ops: [{ action: 'inc', obj: LIST, elemId: dcd3.ops[0].elemId, value: 6, pred: [`${dcd3.startOp}@${D}`] }] })
  r.apply([cd3, ...pads, cb3])
  r.apply([inc3])
  r.set(3, S('over both'))               // two preds, one of them the hidden counter's
  r.apply([new Peer(B, r.changes.slice()).change(d => { d.list[3] = 'again' }), ])
  r.splice(3, 1)
  return finish('counters', 'counters inside a list, one incremented by a hand-encoded change: deletions that reach them and assignments onto them throw; a conflicted element with an incremented counter', r)
}

function pastEnd() {
  const r = new Rec(A)
  r.setup(d => { d.list = [1, 2] })
  r.set(4, S('v'))                       // list[length + 2] = v: two nulls and the value
  r.set(r.length, I(9))                  // list[length] = v: one inserting set
  r.splice(0, r.length)
  r.set(3, ['null', null])               // onto the emptied list: four nulls, one multi-insert at _head
  r.set(r.length + 1, ['bool', true])    // null, true: no datatype on either
  return finish('past_end', 'an assignment past the end of the list: nulls, then the value', r)
}

function bounds() {
  const r = new Rec(A)
  r.setup(d => { d.list = [] })
  r.splice(0, 0)                         // nothing to do, an empty list: no change
  r.splice(0, 1)                         // out of bounds on the empty list
  r.splice(0, 0, [S('a')])
  r.splice(1, 0, [S('b'), S('c')])
  r.splice(3, 0)                         // nothing to do
  r.splice(3, 1)                         // start == length, one deletion
  r.splice(4, 0, [S('y')])               // start > length
  r.splice(1, 5)                         // start + deletions > length
  r.splice(0, r.length)                  // the whole list
  r.splice(0, 0, [S('b'), S('a'), S('c'), S('k')])   // into the emptied list: _head again
  r.splice(0, r.length, [S('x')])        // everything replaced
  return finish('bounds', 'start 0, start == length, the whole list deleted, nothing to do, and the RangeErrors', r)
}

const sessions = [typed(), mixedValues(), twoActors(), conflicts(), holes(), children(), counters(), pastEnd(), bounds()]
const file = path.join(ROOT, 'tests', 'golden', 'list', 'list_splices.json')
fs.mkdirSync(path.dirname(file), { recursive: true })
fs.writeFileSync(file, JSON.stringify({ note: 'tools/fixtures/make_list_splices.js: reference frontend + backend sessions of list.deleteAt / list.insertAt / list[i] = v, with the change requests the frontend produced', sessions }))
for (const s of sessions) console.log(s.name, s.calls.map(c => (c.kind === 'apply' ? 'apply' + c.n : c.kind === 'throws' ? c.error : c.kind + ':' + (c.request ? c.request.ops.length + 'op' : 'nothing'))).join(' '))
console.log(file, fs.statSync(file).size, 'bytes')
