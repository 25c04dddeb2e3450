// TEST INFRASTRUCTURE (build container only: it needs the live reference): the sessions of tests/test_resident_new_objects.py -- calls whose
// batch MAKES objects (am355_set_resident_new_objects), shaped by the reference FRONTEND where it can be (Automerge.change: the op shapes
// applications produce) and by encodeChange where a shape needs it. No generator kind of loggen makes objects inside a session.
// Writes tests/golden/resident/new_objects.json: per session the batches (changes in base64), the reference's incremental patch per call,
// its whole patch at the end, and which calls make objects. Data only.
//   NODE_PATH=oracle/js_shims/node_modules node tools/fixtures/make_new_object_sessions.js
const path = require('path')
const fs = require('fs')
const { loadBackend } = require(path.join(__dirname, '..', '..', 'oracle', 'js', 'ref_loader'))
const ref = loadBackend()
const { Backend, columnar } = ref
const Automerge = ref.Automerge()
const { encodeChange, decodeChange } = columnar
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

// a session: [{ batch: [changes], makes: does the batch make an object, big: its patch is too large to record }]
function record(name, note, calls) {
  let state = Backend.init()
  const patches = []
  for (const call of calls) {
    const r = Backend.applyChanges(state, call.batch)
    state = r[0]
    patches.push(call.big ? null : JSON.stringify(r[1]))   // (a patch of 65 k characters or 300 cards is left to the test's oracle: the file stays in the tens of KB)
  }
  const rows = calls.map(call => call.batch.reduce((n, c) => n + rowsOf(c), 0))
  return { name, note, batches: calls.map(call => call.batch.map(b64)), makes: calls.map(call => !!call.makes), rows, patches,
    whole_patch: calls.some(call => call.big) ? null : JSON.stringify(Backend.getPatch(state)) }
}

const A = id('7'), B = id('9')
const card = k => ({ title: 'card ' + k, done: k % 2 === 0 })

function cards() {
  const a = new Peer(A), calls = []
  const setup = a.change(d => { d.title = new Automerge.Text('t'.repeat(35) + 'u'.repeat(35)); d.cards = [] })   // (a list longer than one wavefront)
  const b = new Peer(B, [setup])
  const hello = b.change(d => { d.hello = 1 })   // (B is an author the document knows from the first call on)
  a.see([hello])
  calls.push({ batch: [setup, hello] })
  for (let k = 0; k < 5; k++) calls.push({ batch: [a.change(d => { d.cards.push(card(k)) })], makes: true })
  calls.push({ batch: [a.change(d => { d.cards.insertAt(0, card(5)) })], makes: true })
  calls.push({ batch: [a.change(d => { d.cards.push({ tags: ['a', 'b'], note: new Automerge.Text('xy') }) })], makes: true })
  calls.push({ batch: [a.change(d => { d.meta = { a: 1 } })], makes: true })
  calls.push({ batch: [a.change(d => { d.log = new Automerge.Text(); d.log.insertAt(0, 'l', 'o', 'g') })], makes: true })
  b.see(calls.slice(1).map(c => c.batch[0]))
  const ca = a.change(d => { d.cards.push(card(6)) }), cb = b.change(d => { d.cards.push(card(7)) })
  a.see([cb]); b.see([ca])
  calls.push({ batch: [ca, cb], makes: true })
  // later calls use what the in-place calls wrote
  calls.push({ batch: [a.change(d => { d.cards[2].title = 'renamed' })] })
  calls.push({ batch: [a.change(d => { d.cards.find(c => c.note).note.insertAt(1, '-', '+') })] })
  calls.push({ batch: [a.change(d => { d.cards.deleteAt(3) })] })
  calls.push({ batch: [a.change(d => { d.cards.find(c => c.tags).tags.push('c') })] })
  calls.push({ batch: [a.change(d => { d.log.insertAt(3, '!'); d.meta.b = 2 })] })
  return record('cards', 'pushes of maps, a nested list and text, makes on map keys, two concurrent pushes; then edits inside what those calls made', calls)
}

function wide() {
  const a = new Peer(A), calls = []
  calls.push({ batch: [a.change(d => { d.list = []; for (let k = 0; k < 130; k++) d.list.push(k) })] })
  calls.push({ batch: [a.change(d => {
    d.list.insertAt(70, -1, card(0), -2)
    d.list.insertAt(20, -3)
    d.list.push(card(1))
  })], makes: true })
  calls.push({ batch: [a.change(d => { d.list.find(x => x.title).title = 'seen'; d.list.insertAt(72, -4) })] })
  return record('wide', 'a list of 130 scalars; one change inserts a card at index 70 with scalars around it, a scalar elsewhere, and a card at the end', calls)
}

function many() {
  const a = new Peer(A), calls = []
  // (4,000 characters, a byte each: more rows than the engine's first guess from the byte count carves, so the first call carves rows + rows / 4 + 65,536, which hold the batch)
  calls.push({ batch: [a.change(d => { d.cards = [card(-1)]; d.title = new Automerge.Text('t'.repeat(4000)) })] })
  calls.push({ batch: [a.change(d => { for (let k = 0; k < 300; k++) d.cards.push({ title: 't' + k, done: false, n: k }) })], makes: true, big: true })
  calls.push({ batch: [a.change(d => { d.cards[299].done = true; d.cards.push(card(300)) })], makes: true })
  return record('many', 'one change pushing 300 cards of three keys: more new objects than one stride of the per-object pass, about 1,200 rows', calls)
}

function declined() {
  const a = new Peer(A), calls = []
  calls.push({ batch: [a.change(d => { d.list = [1, 2, 3, 4, 5]; d.cnt = new Automerge.Counter(0) })] })
  calls.push({ batch: [a.change(d => { d.list[3] = {} })], makes: true })
  calls.push({ batch: [a.change(d => { d.cnt.increment(2); d.list.push({ x: 1 }) })], makes: true })
  return record('declined', 'a list element ASSIGNED an object; a counter increment beside a push', calls)
}

function newcomer() {
  // the newcomer's id sorts in front of the first author's: every kept rank moves
  const a = new Peer(id('c')), calls = []
  const setup = a.change(d => { d.title = new Automerge.Text('title'); d.cards = [card(0)] })
  calls.push({ batch: [setup] })
  const n = new Peer(id('3'), [setup])
  const first = n.change(d => { d.cards.push(card(1)) })
  calls.push({ batch: [first], makes: true })
  a.see([first])
  calls.push({ batch: [a.change(d => { d.cards[1].done = true; d.cards.push(card(2)) })], makes: true })
  return record('newcomer', 'a second actor\'s FIRST change pushes a card; its id sorts in front of the known actor\'s', calls)
}

// a make-call on the row capacity the first call carved (rows + rows / 4 + 65,536, am355_replay.hip carve_cols): `over` rows past it.
// The first call holds 4,000 rows in a few hundred bytes (typing runs of one character: a few dozen bytes per change encoded), far more
// than the rows the engine's first guess from the byte count carves, so the capacity is the formula's.
function capacity(over) {
  const a = new Peer(A), calls = []
  const setup = a.change(d => { d.text = new Automerge.Text('ab'); d.cards = [] })
  const text = Automerge.getObjectId(a.doc.text), d0 = decodeChange(setup)
  let dep = d0.hash, op = d0.startOp + rowsOf(setup), seq = 2, typed = 0
  const typing = rows => {   // changes of up to 4,000 characters, each behind the last one typed
    const out = []
    for (let done = 0; done < rows; seq++) {
      const ops = [], n = Math.min(4000, rows - done)
      for (let k = 0; k < n; k++, op++, typed++) ops.push({ action: 'set', obj: text, elemId: typed === 0 ? '_head' : `${op - 1}@${A}`, insert: true, value: 'z', pred: [] })
      const c = encodeChange({ actor: A, seq, startOp: op - n, time: 0, message: '', deps: [dep], ops })
      dep = decodeChange(c).hash
      out.push(c)
      done += n
    }
    a.see(out)
    return out
  }
  const n0 = 4000, cap = n0 + Math.floor(n0 / 4) + 65536
  calls.push({ batch: [setup].concat(typing(n0 - rowsOf(setup))), big: true })
  const push = 3   // the rows of one pushed card
  calls.push({ batch: typing(cap - n0 - push + over), big: true })
  calls.push({ batch: [a.change(d => { d.cards.push(card(0)) })], makes: true })
  const out = record('capacity' + over, `a pushed card whose rows end ${over} past the row capacity the first call carved`, calls)
  out.capacity = cap
  return out
}

const sessions = [cards(), wide(), many(), declined(), newcomer(), capacity(0), capacity(1)]
const dir = path.join(__dirname, '..', '..', 'tests', 'golden', 'resident')
fs.mkdirSync(dir, { recursive: true })
const file = path.join(dir, 'new_objects.json')
fs.writeFileSync(file, JSON.stringify({ note: 'tools/fixtures/make_new_object_sessions.js: reference frontend sessions whose calls make objects', sessions }))
for (const s of sessions) console.log(s.name, s.batches.length, 'calls, rows', s.rows.join(' '))
console.log(file, fs.statSync(file).size, 'bytes')
