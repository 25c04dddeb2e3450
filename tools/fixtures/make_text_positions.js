// TEST INFRASTRUCTURE (build container only: it needs the live reference): the sessions of tests/test_text_position.py and
// js/test_text_position.js -- elemIds of a Text resolved to POSITIONS, deleted elements included. The reference has no cursor call; the
// number is taken from its public backend by a PROBE: a change of a fresh actor with startOp = maxOp + 1, deps = heads and the one op
// {action: 'set', insert: true, elemId: X, value: '#', pred: []}, applied with Backend.applyChanges(Backend.clone(state), [probe]).
// The probe's op id is the greatest, so it lands directly behind X, in front of X's other children, and the patch reports it at
// index = the caret position behind X. A probe the reference rejects (no such reference element) makes X unknown.
// Writes tests/golden/text/text_positions.json: per session `objectId`, `changes` (every binary change in the order the replica applied
// it, base64), `inserts` ([elemId, the elemId or '_head' it was inserted behind] of every element of the Text, from the decoded changes: what
// a model of the RGA needs) and `checkpoints`, each { n: how many of `changes` were applied, how: 'local' | 'remote' (what the last change was),
// length, refused (the whole-document patch holds a `remove` edit in the Text: the engine refuses such a state),
// queries: [[elemId, status, position, counter]] } with status 'visible' (position = the index, cross-checked against text.getElemId and
// probe index - 1), 'deleted' (position = the probe's index) or 'unknown' (position 0). The queries are EVERY element ever inserted
// into the Text (from the decoded changes, multi-insert `values` expanded), then three that must be unknown: an element of a second
// Text, a counter nobody issued, an actor the document has never seen.
// Data only.
//   NODE_PATH=oracle/js_shims/node_modules node tools/fixtures/make_text_positions.js
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
const A = id('3'), B = id('8'), C = id('d'), PROBE = id('f'), NOBODY = id('e')

function textDiff(diff, objectId) {
  if (diff.objectId === objectId) return diff
  for (const values of Object.values(diff.props || {}))
    for (const v of Object.values(values)) {
      const found = v.objectId ? textDiff(v, objectId) : null
      if (found) return found
    }
  for (const e of diff.edits || []) {
    const found = e.value && e.value.objectId ? textDiff(e.value, objectId) : null
    if (found) return found
  }
  return null
}

class Replica {
  constructor(actor) {
    this.doc = Automerge.init(actor)
    this.changes = []
    this.checkpoints = []
    this.how = 'local'
  }
  get objectId() { return Automerge.getObjectId(this.doc.text) }
  get state() { return Automerge.Frontend.getBackendState(this.doc, 'checkpoint') }
  local(fn) {
    this.doc = Automerge.change(this.doc, { time: 0 }, fn)
    this.changes.push(Automerge.getLastLocalChange(this.doc))
    this.how = 'local'
    return this.changes[this.changes.length - 1]
  }
  remote(batch) {
    const [state, patch] = Backend.applyChanges(this.state, batch)
    this.doc = Automerge.Frontend.applyPatch(this.doc, patch, state)
    this.changes.push(...batch)
    this.how = 'remote'
  }
  // the caret position behind elemId, or null when the reference rejects the probe
  probe(elemId) {
    const state = this.state
    const whole = Backend.getPatch(state)
    const opId = `${whole.maxOp + 1}@${PROBE}`
    const change = encodeChange({ actor: PROBE, seq: 1, startOp: whole.maxOp + 1, time: 0, message: '', deps: Backend.getHeads(state),
      ops: [{ action: 'set', obj: this.objectId, elemId, insert: true, value: '#', pred: [] }] })
    let patch
    try {
      patch = Backend.applyChanges(Backend.clone(state), [change])[1]
    } catch (e) {
      return null
    }
    const diff = textDiff(patch.diffs, this.objectId)
    const edit = diff && diff.edits.find(e => e.opId === opId)
    if (!edit) throw new Error(`the probe behind ${elemId} is not in the patch`)
    return edit.index
  }
  // every element ever inserted into the Text, in the order the changes were applied (pairs: with the element it was inserted behind)
  inserted(pairs = false) {
    const ids = [], after = []
    for (const c of this.changes) {
      const d = decodeChange(c)
      let ctr = d.startOp
      for (const op of d.ops) {
        const n = op.values ? op.values.length : (op.multiOp || 1)
        if (op.insert && op.obj === this.objectId)
          for (let k = 0; k < n; k++) { ids.push(`${ctr + k}@${d.actor}`); after.push(k ? `${ctr + k - 1}@${d.actor}` : op.elemId) }
        ctr += n
      }
    }
    return pairs ? ids.map((x, k) => [x, after[k]]) : ids
  }
  checkpoint() {
    // The frontend asked for text.getElemId is a FRESH one made from the whole-document patch (what Automerge.load shows). The replica's
    // own frontend document can disagree with its backend: text.deleteAt on an element that holds two conflicting values names one pred
    // (frontend/context.js:576-586 for a Text), the other value stays, and the frontend goes on believing the element gone
    // (session `updates`, last checkpoint).
    const objectId = this.objectId
    const whole = Backend.getPatch(this.state)
    const fresh = Automerge.Frontend.applyPatch(Automerge.Frontend.init({ actorId: PROBE, backend: Backend }), whole, this.state)
    const text = fresh.text
    const diff = textDiff(whole.diffs, objectId)
    const refused = diff.edits.some(e => e.action === 'remove')
    // (a `remove` edit in a whole-document patch: the reference's backend goes on counting the element that shows rows but no value, its
    // frontend does not -- text.getElemId no longer agrees with the probe. Such a state records the probe: position = the probe's index
    // less one for an element the fresh frontend shows, and nothing is cross-checked)
    const index = new Map()
    for (let i = 0; i < text.length; i++) index.set(text.getElemId(i), i)
    const queries = []
    if (this.probe('_head') !== 0) throw new Error('_head is not position 0')
    for (const elemId of this.inserted()) {
      const caret = this.probe(elemId)
      if (caret === null) throw new Error(`the reference does not know ${elemId}`)
      if (index.has(elemId)) {
        if (!refused && caret !== index.get(elemId) + 1) throw new Error(`visible ${elemId}: probe ${caret}, index ${index.get(elemId)}`)
        const v = text.get(index.get(elemId))
        queries.push([elemId, 'visible', caret - 1, v instanceof Automerge.Counter ? 1 : 0])
      } else {
        queries.push([elemId, 'deleted', caret, 0])
      }
    }
    const visible = queries.filter(q => q[1] === 'visible').length
    if (visible !== text.length) throw new Error(`${visible} visible elements, length ${text.length}`)
    const other = Automerge.getObjectId(this.doc.other)
    const unknown = [this.doc.other.getElemId(0), `${whole.maxOp + 1000}@${A}`, `2@${NOBODY}`]
    // (a Text no element was ever inserted into: the reference finds no op of the object and places the probe without looking for its
    // reference element at all -- there the probe says nothing, and the three ids are unknown by the definition)
    const empty = this.inserted().length === 0
    for (const elemId of unknown) {
      if (!empty && this.probe(elemId) !== null) throw new Error(`the reference knows ${elemId} (other Text: ${other})`)
      queries.push([elemId, 'unknown', 0, 0])
    }
    this.checkpoints.push({ n: this.changes.length, how: this.how, length: text.length, refused, queries })
  }
}

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

const finish = (name, note, r) => ({ name, note, objectId: r.objectId, changes: r.changes.map(b64), inserts: r.inserted(true), checkpoints: r.checkpoints })
const start = (r, initial) => r.local(d => { d.other = new Automerge.Text('zz'); d.text = initial === undefined ? new Automerge.Text() : new Automerge.Text(initial) })

function typed() {
  const r = new Replica(A)
  start(r)
  r.checkpoint()                                                     // a Text without rows
  r.local(d => d.text.insertAt(0, ...'The quick brown fox'))
  r.checkpoint()
  r.local(d => d.text.insertAt(19, '.'))
  r.local(d => d.text.insertAt(4, ...'very '))
  r.checkpoint()
  r.local(d => d.text.deleteAt(3, 4))
  r.checkpoint()
  r.local(d => d.text.deleteAt(0, 2))                                // the first elements: deleted at 0
  r.local(d => d.text.deleteAt(d.text.length - 2, 2))                // the last ones: deleted at the length
  r.checkpoint()
  r.local(d => d.text.insertAt(0, '>'))
  r.local(d => d.text.insertAt(d.text.length, ...' end'))
  r.checkpoint()
  return finish('typed', 'one actor: pasted runs, keystrokes, deletions inside a run, at the head and at the end', r)
}

function twoActors() {
  const r = new Replica(A)
  const setup = start(r, 'hello world')
  const b = new Peer(B, [setup])
  const del = r.local(d => d.text.deleteAt(3, 4))                    // hel|orld
  const ins = b.change(d => d.text.insertAt(5, 'X', 'Y'))            // before it has seen the deletion: helXYorld
  r.checkpoint()
  r.remote([ins])
  r.checkpoint()
  b.see([del])
  // interleaved concurrent inserts at the same place, three rounds
  for (let k = 0; k < 3; k++) {
    const ca = r.local(d => d.text.insertAt(2, String.fromCharCode(97 + k), String.fromCharCode(65 + k)))
    const cb = b.change(d => d.text.insertAt(2, String(k)))
    r.remote([cb]); b.see([ca])
    r.checkpoint()
  }
  const c = new Peer(C, r.changes)
  const cc = c.change(d => { d.text.deleteAt(1, 5); d.text.insertAt(1, 'c') })
  const cb = b.change(d => d.text.deleteAt(0, 3))
  r.remote([cc, cb])
  r.checkpoint()
  return finish('two_actors', 'an insertion concurrent with a deletion around it (the issue\'s helXYorld), interleaved concurrent inserts at one place, a third actor', r)
}

function holes() {
  const r = new Replica(A)
  const setup = start(r)
  const paste = r.local(d => d.text.insertAt(0, ...'0123456789abcdefghijklmnopqrstuvwxyz'))
  const b = new Peer(B, [setup, paste])
  r.local(d => d.text.deleteAt(10, 3))                               // holes inside the pasted run
  r.local(d => d.text.deleteAt(20, 1))
  r.checkpoint()
  const foreign = b.change(d => d.text.insertAt(6, 'P', 'Q'))        // another actor's elements inside the run, between `5` and `6`
  r.remote([foreign])
  r.checkpoint()
  r.local(d => d.text.deleteAt(6, 2))                                // ... deleted: `5` and `6` are one record again, two tombstones between them
  r.checkpoint()
  const more = b.change(d => d.text.insertAt(3, 'R'))
  r.remote([more])
  r.local(d => d.text.deleteAt(3, 1))
  r.local(d => d.text.deleteAt(0, 1))
  r.checkpoint()
  return finish('holes', 'deletions inside a pasted multi-insert run; another actor\'s insertion inside the run, then deleted: a tombstone between two values of one record', r)
}

function updates() {
  const r = new Replica(A)
  const setup = start(r, 'abcdefghij')
  const b = new Peer(B, [setup])
  r.local(d => d.text.set(4, 'X'))
  r.checkpoint()
  const cb = b.change(d => d.text.set(4, 'Y'))                       // concurrent: two values on one element
  r.remote([cb])
  r.checkpoint()
  r.local(d => d.text.set(9, '1'))                                   // the last element of the run
  r.local(d => d.text.set(0, 'A'))                                   // the first
  r.checkpoint()
  r.local(d => d.text.deleteAt(3, 3))                                // over the conflicting element
  r.local(d => d.text.insertAt(3, ...'new'))
  r.local(d => d.text.set(4, 'E'))
  r.checkpoint()
  return finish('updates', 'text.set(i, v): update records, a conflict of two actors on one element, assignments to the first and the last element of a run', r)
}

function allDeleted() {
  const r = new Replica(A)
  const setup = start(r, 'gone soon')
  const b = new Peer(B, [setup])
  const cb = b.change(d => d.text.insertAt(4, '!'))
  r.local(d => d.text.deleteAt(0, 9))
  r.checkpoint()                                                     // rows, no records
  r.remote([cb])                                                     // one element among the tombstones
  r.checkpoint()
  r.local(d => d.text.deleteAt(0, 1))
  r.checkpoint()
  r.local(d => d.text.insertAt(0, ...'back'))
  r.checkpoint()
  return finish('all_deleted', 'the whole Text deleted: every element is deleted at 0; typed into again', r)
}

// the ids of the counters a change inserted into the Text
function counterIds(change, objectId) {
  const s = decodeChange(change), ids = []
  let ctr = s.startOp
  for (const op of s.ops) {
    const n = op.values ? op.values.length : 1
    if (op.datatype === 'counter' && op.obj === objectId && op.insert) for (let k = 0; k < n; k++) ids.push(`${ctr + k}@${s.actor}`)
    ctr += n
  }
  return { ids, next: ctr, hash: s.hash }
}

function counters() {
  const r = new Replica(A)
  start(r, 'ab')
  const made = r.local(d => { d.text.insertAt(1, new Automerge.Counter(3)); d.text.insertAt(3, 'c', new Automerge.Counter(7), 'd') })
  const { ids, next, hash } = counterIds(made, r.objectId)
  if (ids.length !== 2) throw new Error('no two counters in the change')
  r.checkpoint()                                                     // a C3 b c C7 d
  // the frontend cannot increment a counter inside a Text: the increment is encoded by hand (the approach of text_reads.json)
  const inc = encodeChange({ actor: B, seq: 1, startOp: next, time: 0, message: '', deps: [hash],
    ops: [{ action: 'inc', obj: r.objectId, elemId: ids[1], value: 5, pred: [ids[1]] }] })
  r.remote([inc])
  r.checkpoint()
  r.local(d => d.text.deleteAt(0, 1))
  r.local(d => d.text.insertAt(2, '+'))
  r.checkpoint()
  return finish('counters', 'counters inside a Text, one incremented by a hand-encoded change: the counter flag of visible elements', r)
}

function removeRecord() {
  const r = new Replica(A)
  start(r, 'ab')
  const made = r.local(d => d.text.insertAt(1, new Automerge.Counter(3), 'x'))
  const { ids, next, hash } = counterIds(made, r.objectId)
  if (ids.length !== 1) throw new Error('no counter in the change')
  r.checkpoint()
  r.local(d => d.text.deleteAt(1, 1))                                // the counter deleted ...
  r.checkpoint()
  const inc = encodeChange({ actor: B, seq: 1, startOp: next, time: 0, message: '', deps: [hash],   // ... and incremented by somebody who has not seen that
    ops: [{ action: 'inc', obj: r.objectId, elemId: ids[0], value: 5, pred: [ids[0]] }] })
  // (through the backend alone: what the frontend makes of the incremental patch is not the subject)
  const state = Backend.applyChanges(r.state, [inc])[0]
  r.doc = Automerge.Frontend.applyPatch(Automerge.Frontend.init({ actorId: A, backend: Backend }), Backend.getPatch(state), state)
  r.changes.push(inc)
  r.how = 'remote'
  r.checkpoint()
  return finish('remove_record', 'an increment of a deleted counter inside the Text: the whole-document patch holds a `remove` edit, the state the engine refuses', r)
}

const sessions = [typed(), twoActors(), holes(), updates(), allDeleted(), counters(), removeRecord()]
const file = path.join(ROOT, 'tests', 'golden', 'text', 'text_positions.json')
fs.mkdirSync(path.dirname(file), { recursive: true })
fs.writeFileSync(file, JSON.stringify({ note: 'tools/fixtures/make_text_positions.js: elemIds of a Text and their positions by the probe on the reference backend', sessions }))
for (const s of sessions)
  console.log(s.name, s.checkpoints.map(c => `${c.n}:${c.refused ? 'refused ' : ''}${c.queries.filter(q => q[1] === 'visible').length}v/${c.queries.filter(q => q[1] === 'deleted').length}d`).join(' '))
console.log(file, fs.statSync(file).size, 'bytes')
