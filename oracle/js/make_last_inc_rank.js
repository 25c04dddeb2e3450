// TEST INFRASTRUCTURE (build container only): a session in which the actor RANK inside a counter's stored last-increment id is observable
// after newcomers have moved it (tests/test_resident_new_actors.py). Actors A < N1 < N2 < B by id. A and B increment the counter
// 1@X concurrently, both with op counter 5: the counter is complete at its last increment, 5@B. Then N1 and N2 arrive in one batch, and
// N2 assigns the same key concurrently under 5@N2: the key has two values, emitted in the order of (5@N2, 5@B) -- equal counters, so by
// the actors alone. B's rank was 2 when 5@B was stored and is 4 now; N2's is 3.
// Writes tests/golden/resident/last_inc_rank.json: the batches (changes in base64) and the reference's patches, for the record -- the
// test compares with the sequential oracle.
//   NODE_PATH=oracle/js_shims/node_modules node oracle/js/make_last_inc_rank.js
const { loadBackend } = require('./ref_loader')
const { Backend, columnar } = loadBackend()
const { encodeChange, decodeChange } = columnar
const fs = require('fs')
const path = require('path')
const id = d => d.repeat(32)
const X = id('1'), A = id('2'), N1 = id('4'), N2 = id('5'), B = id('8')
function mk(actor, seq, startOp, deps, ops) { return encodeChange({actor, seq, startOp, time: 0, message: '', deps, ops}) }
const hashOf = c => decodeChange(c).hash
const c1 = mk(X, 1, 1, [], [{action: 'set', obj: '_root', key: 'cnt', value: 10, datatype: 'counter', pred: []},
  {action: 'set', obj: '_root', key: 'plain', value: 1, datatype: 'int', pred: []}])
const cA = mk(A, 1, 5, [hashOf(c1)], [{action: 'inc', obj: '_root', key: 'cnt', value: 1, pred: ['1@' + X]}])
const cB = mk(B, 1, 5, [hashOf(c1)], [{action: 'inc', obj: '_root', key: 'cnt', value: 2, pred: ['1@' + X]}])
const cN1 = mk(N1, 1, 3, [hashOf(c1)], [{action: 'set', obj: '_root', key: 'other', value: 4, datatype: 'int', pred: []}])
const cN2 = mk(N2, 1, 5, [hashOf(c1)], [{action: 'set', obj: '_root', key: 'cnt', value: 'v', pred: []}])
const cA2 = mk(A, 2, 6, [hashOf(cA)], [{action: 'set', obj: '_root', key: 'plain', value: 2, datatype: 'int', pred: ['2@' + X]}])
const batches = [[c1, cA, cB], [cN1, cN2], [cA2]]
const b64 = u8 => Buffer.from(u8.buffer, u8.byteOffset, u8.byteLength).toString('base64')
let state = Backend.init()
const patches = []
for (const b of batches) {
  const r = Backend.applyChanges(state, b)
  state = r[0]
  patches.push(JSON.stringify(r[1]))
}
const out = { name: 'last_inc_rank', note: 'hand-built changes via reference encodeChange: two values of one key ordered by the actor of a counter\'s last increment',
  actors: { X, A, N1, N2, B }, batches: batches.map(b => b.map(b64)), patches, whole_patch: JSON.stringify(Backend.getPatch(state)) }
const dir = path.join(__dirname, '..', '..', 'tests', 'golden', 'resident')
fs.mkdirSync(dir, { recursive: true })
fs.writeFileSync(path.join(dir, 'last_inc_rank.json'), JSON.stringify(out))
console.log(patches[1])
console.log(out.whole_patch)
