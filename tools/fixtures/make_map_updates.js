// TEST INFRASTRUCTURE (build container only: it needs the live reference): the sessions of tests/test_map_update.py and
// js/test_map_update.js -- a MAP edited by KEY. The reference FRONTEND + the reference BACKEND execute
// Automerge.change(doc, {time}, d => { d.a = v; delete d.b; d.n.increment(k) }) on _root, a nested map or a table; the backend of the
// recorded replica is a stub that records the change REQUEST the frontend hands to applyLocalChange before passing it on.
// Writes tests/golden/map/map_updates.json: per session `changes` (every binary change of the session in the order it was applied,
// base64) and `calls`, each with n_before = how many of `changes` were applied before it:
//   { kind: 'apply', n }            the next n changes arrive through Backend.applyChanges (the setup, other actors' edits)
//   { kind: 'update', objectId, table, ops, actor, time, request, change, patch, object }
//                                   one Automerge.change on one map: ops = [['set', key, [class, v]] | ['del', key] | ['inc', key, delta]] in
//                                   the order they were made; the request the frontend produced, the binary change, the patch
//                                   applyLocalChange returned (JSON text) and the object afterwards (JSON text). request / change / patch
//                                   are null where the frontend made no change (deletions of absent keys only). table: the object is a
//                                   Table and ['del', rowId] is table.remove(rowId)
//   { kind: 'throws', ...its arguments, error, message }
//                                   a call the frontend throws on: the class and text of its exception; the state stays
// An increment of a key that holds no Counter cannot be written with the proxies (there is no increment() to call): the generator calls
// context.increment, which a Counter's increment() calls, on the change's context, so that the exception is the reference's own.
// VALUES are written as [class, v] pairs, as in make_list_splices.js. Every recorded `set` is one the reference emits an op for (it skips
// an assignment of the value a key already shows without a conflict; the generator fails on such a call).
// Data only.
//   NODE_PATH=oracle/js_shims/node_modules node tools/fixtures/make_map_updates.js
const path = require('path')
const fs = require('fs')
const ROOT = path.join(__dirname, '..', '..')
const { loadBackend, REF } = require(path.join(ROOT, 'oracle', 'js', 'ref_loader'))
const { CHANGE } = require(path.join(REF, 'frontend', 'constants'))
const ref = loadBackend()
const { Backend, columnar } = ref
const Automerge = ref.Automerge()
const { decodeChange, encodeChange } = columnar
const id = d => d.repeat(32 / d.length)
const b64 = u8 => Buffer.from(u8.buffer, u8.byteOffset, u8.byteLength).toString('base64')
const copy = x => JSON.parse(JSON.stringify(x))

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
const set = (k, v) => ['set', k, v], del = k => ['del', k], inc = (k, n) => ['inc', k, n]

// The recorded replica: its frontend document sits on the reference backend through a stub that keeps the last request. `at`: the map
// that is edited, as a function of the document (d => d for _root).
class Rec {
  constructor(actor, at = d => d, table = false) {
    this.actor = actor
    this.at = at
    this.table = table
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
  get objectId() { return Automerge.getObjectId(this.at(this.doc)) }
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
  update(...ops) {
    const time = ++this.clock
    const call = { objectId: this.objectId, table: this.table, ops, actor: this.actor, time, n_before: this.changes.length }
    this.last = null
    try {
      this.doc = Automerge.change(this.doc, { time }, d => {
        const o = this.at(d)
        for (const op of ops) {
          if (op[0] === 'set') o[op[1]] = js(op[2])
          else if (op[0] === 'del' && this.table) o.remove(op[1])
          else if (op[0] === 'del') delete o[op[1]]
          else if (o[op[1]] instanceof Automerge.Counter) o[op[1]].increment(op[2])
          else {   // (no Counter there: no proxy has an increment() to call -- context.increment itself, the method a Counter's calls)
            if (this.objectId !== '_root') throw new Error('increments of what is no counter are recorded on _root only')
            d[CHANGE].increment([], op[1], op[2])
          }
        }
      })
    } catch (e) {
      if (!(e instanceof RangeError) && !(e instanceof TypeError)) throw e
      this.calls.push(Object.assign({ kind: 'throws' }, call, { error: e instanceof RangeError ? 'RangeError' : 'TypeError', message: e.message }))
      return null
    }
    const made = this.last
    for (const op of ops)
      if (op[0] !== 'del' && !(made && made.request.ops.some(r => r.key === op[1] && r.action === op[0])))
        throw new Error(`the reference emitted no op for ${JSON.stringify(op)}: not recorded, choose another value`)
    this.calls.push(Object.assign({ kind: 'update' }, call, { request: made && made.request, change: made && b64(made.change), patch: made && made.patch,
      object: JSON.stringify(this.at(this.doc)) }))
    if (made) this.changes.push(made.change)
    return made && made.change
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

const finish = (name, note, rec) => ({ name, note, changes: rec.changes.map(b64), calls: rec.calls })
const A = id('3'), B = id('8'), C = id('d'), D = id('5')

function root() {
  const r = new Rec(A)
  r.update(set('title', S('hello')))                         // the first change of the document
  r.update(set('n', I(1)), set('flag', ['bool', true]))      // two ops in one change
  r.update(set('title', S('hello, world')))                  // an overwrite: one pred
  r.update(del('flag'))
  r.update(del('flag'))                                      // absent now: no op, no change
  r.update(del('never'))                                     // never there
  r.update(set('flag', ['bool', false]))                     // a deleted key set again: no pred
  r.update(set('a', I(1)), del('n'), set('z', S('last')), del('nothing'), set('m', ['null', null]))   // several ops, one of them without effect
  r.update(del('a'), del('m'), del('z'))
  r.update(set('title', S('')))                              // an empty string value
  return finish('root', '_root of one actor: keys set, overwritten, deleted, deleted again (no op), set again, several ops in one change', r)
}

function nested() {
  const r = new Rec(A, d => d.config)
  r.setup(d => { d.config = { a: 1, inner: { c: 2 } }; d.other = { a: 'not this one' } })
  r.update(set('a', I(2)))
  r.update(set('b', S('new')), del('a'))
  const r2 = new Rec(B, d => d.config.inner)
  r2.apply(r.changes.slice())
  r2.update(set('c', I(3)), set('d', ['float64', 2.5]))
  r2.update(del('c'))
  return [finish('nested', 'a map inside _root, beside another map that holds the same key', r), finish('nested_inner', 'a map two levels down, edited by a second actor', r2)]
}

function conflicts() {
  const a = new Peer(A)
  const setup = a.change(d => { d.k2 = 'base2'; d.k3 = 'base3'; d.solo = 'base' })
  const b = new Peer(B, [setup]), e = new Peer(D, [setup])
  const c2 = [a.change(d => { d.k2 = 'a2' }), b.change(d => { d.k2 = 'b2' })]                                        // two values
  const c3 = [a.change(d => { d.k3 = 'a3' }), b.change(d => { d.k3 = 'b3' }), e.change(d => { d.k3 = 'e3' })]        // three values
  const cn = [b.change(d => { d.fresh = 1 }), e.change(d => { d.fresh = 2 })]                                         // a key both make
  const r = new Rec(C)
  r.apply([setup])
  r.apply([...c2, ...c3, ...cn])
  r.update(set('k2', S('won')))            // two preds
  r.update(del('k3'))                      // three preds
  r.update(set('fresh', I(3)), set('solo', S('mine')))
  // remote changes between the calls: a fresh conflict of three on the key just resolved, and a concurrent overwrite of the replica's own value
  const now = r.changes.slice()
  const a2 = new Peer(A, now), b2 = new Peer(B, now), e2 = new Peer(D, now)
  r.apply([a2.change(d => { d.k2 = 'u' }), b2.change(d => { d.k2 = 'v' }), e2.change(d => { d.k2 = 'w' })])
  r.update(set('other', I(0)))             // beside the conflict
  r.update(set('k2', S('won')))            // the value it had: emitted all the same, it resolves a conflict (three preds)
  r.apply([a2.change(d => { d.k3 = 'back' })])   // the deleted key set by a remote actor
  r.update(del('k3'), del('k2'))
  return finish('conflicts', 'two and three actors assign one key concurrently; the key is then assigned, deleted, and conflicted again by remote changes between the calls', r)
}

function counters() {
  const a = new Peer(A)
  // votes: a counter; cc: two actors assign a Counter concurrently; cw: a Counter (the greater op id: shown) beside a string; pw: a string (shown) beside a Counter
  const setup = a.change(d => { d.votes = new Automerge.Counter(0); d.cc = 0; d.cw = 0; d.pw = 0; d.plain = 'p' })
  const b = new Peer(B, [setup])
  const ca = a.change(d => { d.cc = new Automerge.Counter(10); d.cw = 'string of a'; d.pw = new Automerge.Counter(7) })
  const cb = b.change(d => { d.cc = new Automerge.Counter(20); d.cw = new Automerge.Counter(5); d.pw = 'string of b' })
  const r = new Rec(C)
  r.apply([setup])
  r.update(inc('votes', 1))
  r.update(inc('votes', 5), set('beside', I(1)))   // an increment beside an assignment
  r.update(inc('votes', -3))                   // a decrement
  r.update(set('votes', I(0)))                 // RangeError: onto a counter
  r.update(inc('plain', 1))                    // TypeError: no counter
  r.update(inc('absent', 1))                   // TypeError: no such key
  r.update(set('ok', I(1)), inc('plain', 1))   // the second op throws: the whole change is dropped
  r.apply([ca, cb])
  r.update(inc('cc', 1))                       // a conflicted counter: two preds, the shown one is b's
  r.update(inc('cw', 2))                       // counter beside a string, the counter wins: two preds
  r.update(set('cw', S('x')))                  // RangeError: the shown value is the counter
  r.update(inc('pw', 1))                       // TypeError: the string wins
  r.update(set('pw', S('resolved')))           // two preds, one of them the hidden counter's
  r.update(del('votes'))                       // a counter may be deleted
  r.update(set('votes', ['counter', 100]))     // and made again
  r.update(inc('votes', 1))
  r.update(del('cc'))
  return finish('counters', 'map counters: increments, a conflicted counter, a counter beside a plain value where each wins in turn, and the calls that throw', r)
}

function children() {
  const a = new Peer(A)
  const setup = a.change(d => { d.child = { x: 1 }; d.list = [1, 2]; d.text = new Automerge.Text('ab'); d.keep = { y: 2 } })
  const b = new Peer(B, [setup])
  const cb = b.change(d => { d.keep = 'b overwrote the map' })          // a child object beside a primitive: b's string ...
  const ca = a.change(d => { d.keep = { y: 3 } })                       // ... and, concurrently, a's new map
  const r = new Rec(C)
  r.apply([setup])
  r.update(set('child', S('was a map')))       // a key holding a child object, overwritten: the pred is the make op
  r.update(del('list'))                        // deleted
  r.update(set('text', I(7)), set('child', S('again')))
  r.apply([cb, ca])
  r.update(set('keep', I(0)))                  // over a map and a string: two preds
  return finish('children', 'keys that hold child objects (a map, a list, a Text) overwritten and deleted', r)
}

function table() {
  const a = new Peer(A)
  let rows = []
  const setup = a.change(d => { d.books = new Automerge.Table(); rows.push(d.books.add({ title: 'one' })); rows.push(d.books.add({ title: 'two' })); rows.push(d.books.add({ title: 'three' })) })
  const r = new Rec(C, d => d.books, true)
  r.apply([setup])
  r.update(del(rows[1]))
  r.update(del(rows[0]), del(rows[2]))
  return finish('table', 'rows of a Table removed by their id', r)
}

function keyOrder() {
  // prefixes of each other; U+E000 - U+FFFF beside supplementary-plane characters (UTF-16 order != byte order); long keys
  const keys = ['a', 'ab', 'abc', 'abcd', 'b', 'x', '\uE000', '\uE000x', '\uFFFF', '\uFFFD', '\u{10000}', '\u{1F600}', '\u{10FFFF}', 'z', '\u00E9', '\u00E9a', '\uD7FF',
    'k'.repeat(300), 'k'.repeat(300) + 'a', 'k'.repeat(299)]
  const r = new Rec(A)
  r.setup(d => { keys.forEach((k, i) => { d[k] = i }) })
  keys.forEach((k, i) => { if (i % 3 === 0) r.update(set(k, I(1000 + i))) })
  r.update(...keys.filter((_, i) => i % 3 === 1).map(k => del(k)))
  r.update(...keys.filter((_, i) => i % 3 === 2).map((k, i) => set(k, S('v' + i))))
  r.update(set('abcde', I(1)), set('\u{10001}', I(2)), set('\uE001', I(3)), del('ab'), del('\uFFFE'))   // new keys between the old ones, absent ones deleted
  keys.forEach((k, i) => { if (i % 3 !== 1) r.update(del(k)) })
  return finish('key_order', 'keys that are prefixes of each other, keys of U+E000..U+FFFF beside supplementary-plane characters, keys longer than 256 bytes', r)
}

function mixedValues() {
  const r = new Rec(A)
  r.update(set('s', S('\u00E9\u20AC\u{1F600}')), set('t', ['bool', true]), set('f', ['bool', false]), set('n', ['null', null]))
  r.update(set('i', I(-5)), set('u', ['uint', 7]), set('d', ['float64', 2.5]), set('d3', ['float64', 3]))
  r.update(set('ts', ['timestamp', 1600000000000]), set('c', ['counter', 3]), set('big', I(9007199254740991)))
  r.update(set('s', I(1)), set('i', S('now a string')), set('n', ['timestamp', 5]), set('d', ['null', null]))
  r.update(inc('c', 4))
  return finish('mixed_values', 'values of every class assigned and overwritten by another class', r)
}

function bounds() {
  const r = new Rec(A)
  r.update(set('', I(1)))                      // RangeError: an empty key
  r.update(del(''))                            // no op
  r.update(inc('', 1))                         // TypeError
  r.update(set('a', I(1)))
  r.update(set('b', I(2)), set('', I(3)))      // the second op throws: the change is dropped
  r.update(set('b', I(2)))                     // the state is still served
  return finish('bounds', 'the empty key, and a change whose later op throws', r)
}

const sessions = [root(), ...nested(), conflicts(), counters(), children(), table(), keyOrder(), mixedValues(), bounds()]
const file = path.join(ROOT, 'tests', 'golden', 'map', 'map_updates.json')
fs.mkdirSync(path.dirname(file), { recursive: true })
fs.writeFileSync(file, JSON.stringify({ note: 'tools/fixtures/make_map_updates.js: reference frontend + backend sessions of map assignments, deletions and increments, with the change requests the frontend produced', sessions }))
for (const s of sessions) console.log(s.name, s.calls.map(c => (c.kind === 'apply' ? 'apply' + c.n : c.kind === 'throws' ? c.error : c.kind + ':' + (c.request ? c.request.ops.length + 'op' : 'nothing'))).join(' '))
console.log(file, fs.statSync(file).size, 'bytes')
