// TEST INFRASTRUCTURE (build container only: it needs the live reference): the hand-shaped change requests of tests/test_local_small.py --
// the smallest shapes at which the one-workgroup encoder of a small local change (csrc/am355_hist.hip kl_small) can go wrong: the state
// transitions of every column kind (run, literal, null run; numbers, deltas, strings, booleans), every value tag, the LEB128 length
// boundaries, multi-ops at the wavefront edges, the pred order, and requests on and one past each of the path's limits.
// Writes tests/golden/local/small_edges.json: per entry { name, request, change (base64, as encodeChange returns it), hash } -- made by the
// reference's own encodeChange. Data only. A request with seq > 1 carries its full deps: encodeChange adds none.
//   NODE_PATH=oracle/js_shims/node_modules node tools/fixtures/make_local_small_edges.js
const path = require('path')
const fs = require('fs')
const ROOT = path.join(__dirname, '..', '..')
const { loadBackend } = require(path.join(ROOT, 'oracle', 'js', 'ref_loader'))
const { columnar } = loadBackend()
const { encodeChange, decodeChange } = columnar
const id = d => d.repeat(32 / d.length)
const A = id('7'), B = id('9'), C = id('b')
// the limits of the path (csrc/am355_hist.h LOCAL_SMALL_*), for the entries on and one past them
const ROWS = 512, PREDS = 512, OPS = 256, BYTES = 4096

const entries = []
function add(name, ops, more = {}) {
  const request = Object.assign({ actor: A, seq: 1, startOp: 1, time: 0, message: '', deps: [], ops }, more)
  const bin = encodeChange(JSON.parse(JSON.stringify(request)))
  entries.push({ name, request, change: Buffer.from(bin.buffer, bin.byteOffset, bin.byteLength).toString('base64'), hash: decodeChange(bin).hash })
  return bin
}
const setKey = (key, value, more = {}) => Object.assign({ action: 'set', obj: '_root', key, value, pred: [] }, more)
const mixed = n => Array.from({ length: n }, (_, k) => ['a', 'é', '€', '𝄞', 'z'][k % 5])   // UTF-8 of 1, 2, 3, 4, 1 bytes

add('empty_change', [])
add('one_root_set', [setKey('k', 1)])
add('type_own_elem', [{ action: 'set', obj: `1@${A}`, elemId: `5@${A}`, insert: true, value: 'x', pred: [] }], { seq: 2, startOp: 6, deps: ['ab'.repeat(32)] })
add('type_other_elem', [{ action: 'set', obj: `1@${A}`, elemId: `5@${B}`, insert: true, value: 'x', pred: [] }], { startOp: 6 })

// ---- the state transitions, per column kind. A pattern is a string of symbols; equal symbols give equal values, `_` a null ----
const PATTERNS = { run2: 'aa', lit2: 'ab', abb: 'abb', aab: 'aab', run_lit_run: 'aabcdd', null_middle: 'aa_bc', null_leading: '__ab', null_trailing: 'ab__' }
const sym = ch => ch.charCodeAt(0) - 97
for (const [name, pat] of Object.entries(PATTERNS)) {
  // numbers: objActor, objCtr, keyActor, action, valLen, predNum and the boolean `insert` follow the pattern (`_`: a map-key row on the root)
  add(`num_${name}`, [...pat].map(ch => {
    if (ch === '_') return setKey('k', null)
    const k = sym(ch)
    const op = { action: k === 3 ? 'del' : 'set', obj: `${k + 1}@${k % 2 ? B : A}`, elemId: `${5 * (k + 1)}@${k % 2 ? A : C}`, insert: k % 2 === 0,
      pred: Array.from({ length: k + 1 }, (_, j) => `${j + 1}@${A}`) }
    if (op.action === 'set') op.value = 'v'.repeat(k + 1)
    if (op.action === 'del') op.insert = false
    return op
  }), { startOp: 40 })
  // deltas: keyCtr and predCtr step by the pattern's symbol (a +3, b +7, c -2, d +1); `_`: a map-key row, null in keyCtr, nothing in predCtr
  let ctr = 20
  add(`delta_${name}`, [...pat].map(ch => {
    if (ch === '_') return setKey('k', true)
    ctr += [3, 7, -2, 1][sym(ch)]
    return { action: 'del', obj: `1@${A}`, elemId: `${ctr}@${A}`, pred: [`${ctr}@${A}`] }
  }), { startOp: 60 })
  // strings: keyStr follows the pattern (`_`: a list row, null in keyStr)
  add(`key_${name}`, [...pat].map(ch => ch === '_' ? { action: 'del', obj: `1@${A}`, elemId: `2@${A}`, pred: [`2@${A}`] } : setKey(`key-${ch}`, sym(ch))), { startOp: 9 })
}
const long = 'L'.repeat(199)
add('key_200_bytes', [setKey(long + 'x', 1), setKey(long + 'x', 2), setKey(long + 'y', 3)])
add('key_multibyte', ['é', 'é', '€', '𝄞', '𝄞', 'e'].map((k, i) => setKey(k, i)))
add('key_same_first_16', ['0123456789abcdefX', '0123456789abcdefY', '0123456789abcdefY', '0123456789abcdef'].map((k, i) => setKey(k, i)))

add('every_value_tag', [
  setKey('null', null), setKey('true', true), setKey('false', false), setKey('uint', 300, { datatype: 'uint' }), setKey('negint', -7),
  setKey('float', 1.5), setKey('float_whole', 3, { datatype: 'float64' }), setKey('empty', ''), setKey('s1', 'a'), setKey('s2', 'é'), setKey('s3', '€'), setKey('s4', '𝄞'),
  setKey('smix', 'aé€𝄞'), setKey('counter', 10, { datatype: 'counter' }), setKey('timestamp', 1234567890123, { datatype: 'timestamp' })])
add('leb128_edges', [63, 64, 127, 128, -64, -65, 2 ** 53 - 1, -(2 ** 53 - 1)].map((v, i) => setKey(`n${i}`, v))
  .concat([63, 64, 127, 128, 2 ** 53 - 1].map((v, i) => setKey(`u${i}`, v, { datatype: 'uint' }))))
for (const n of [63, 64, 65, 128]) add(`multi_insert_${n}`, [{ action: 'set', obj: `1@${A}`, elemId: '_head', insert: true, values: mixed(n), pred: [] }], { startOp: 2 })
add('multi_delete_70', [{ action: 'del', obj: `1@${A}`, elemId: `4@${A}`, multiOp: 70, pred: [`4@${A}`] }], { startOp: 200 })
add('five_preds_three_actors', [setKey('k', 'v', { pred: [`9@${C}`, `3@${B}`, `9@${A}`, `3@${A}`, `9@${B}`] })], { startOp: 20 })
add('counters_go_down', [
  { action: 'del', obj: `1@${A}`, elemId: `90@${A}`, pred: [`90@${A}`] }, { action: 'del', obj: `1@${A}`, elemId: `40@${B}`, pred: [`40@${B}`] },
  setKey('k', 1), { action: 'del', obj: `1@${A}`, elemId: `39@${A}`, pred: [`39@${A}`] }, setKey('j', 2, { pred: [`7@${A}`] }),
  { action: 'set', obj: `1@${A}`, elemId: `2@${B}`, insert: true, value: 'x', pred: [] }, { action: 'del', obj: `1@${A}`, elemId: `1000000@${A}`, pred: [`3@${B}`, `1000000@${A}`] }], { startOp: 100 })
add('make_map_and_sets', [{ action: 'makeMap', obj: '_root', key: 'm', pred: [] }, { action: 'set', obj: `1@${A}`, key: 'a', value: 1, pred: [] }, { action: 'set', obj: `1@${A}`, key: 'b', value: 2, pred: [] }])
add('make_text_and_insert', [{ action: 'makeText', obj: '_root', key: 't', pred: [] }, { action: 'set', obj: `1@${A}`, elemId: '_head', insert: true, values: ['h', 'i', '!'], pred: [] }])
add('make_list_and_table', [{ action: 'makeList', obj: '_root', key: 'l', pred: [] }, { action: 'makeTable', obj: '_root', key: 't', pred: [] }])
add('inc', [{ action: 'inc', obj: '_root', key: 'c', value: 3, pred: [`4@${B}`] }], { startOp: 9 })
add('del_key', [{ action: 'del', obj: '_root', key: 'gone', pred: [`4@${A}`] }], { startOp: 9 })
{
  // the two sides of DEFLATE_MIN_SIZE = 256 bytes: byte 8 of the container is 1 (plain) below it and 2 (DEFLATEd) from it on
  const insert = n => [{ action: 'set', obj: `1@${A}`, elemId: '_head', insert: true, values: Array.from({ length: n }, (_, k) => 'é' + (k % 7)), pred: [] }]
  let n = 1
  while (encodeChange({ actor: A, seq: 1, startOp: 2, time: 0, message: '', deps: [], ops: insert(n) })[8] === 1) n++
  add('container_below_256', insert(n - 1), { startOp: 2 })
  add('container_above_256', insert(n), { startOp: 2 })
}

// ---- on and one past each limit ----
const typed = n => [{ action: 'set', obj: `1@${A}`, elemId: '_head', insert: true, values: Array.from({ length: n }, (_, k) => String.fromCharCode(97 + k % 26)), pred: [] }]
add('limit_rows_on', typed(ROWS), { startOp: 2 })
add('limit_rows_past', typed(ROWS + 1), { startOp: 2 })
const twoPreds = extra => Array.from({ length: PREDS / 2 }, (_, k) => setKey('k', true, { pred: [`${k + 1}@${A}`, `${k + 1}@${B}`].concat(k === 0 && extra ? [`${k + 2}@${B}`] : []) }))
add('limit_preds_on', twoPreds(false), { startOp: 2000 })
add('limit_preds_past', twoPreds(true), { startOp: 2000 })
add('limit_ops_on', Array.from({ length: OPS }, (_, k) => setKey('k', k % 3 === 0)))
add('limit_ops_past', Array.from({ length: OPS + 1 }, (_, k) => setKey('k', k % 3 === 0)))
add('limit_bytes_on', [setKey('K'.repeat(96), 'v'.repeat(BYTES - 96))])
add('limit_bytes_past', [setKey('K'.repeat(96), 'v'.repeat(BYTES - 96 + 1))])

const dir = path.join(ROOT, 'tests', 'golden', 'local')
fs.mkdirSync(dir, { recursive: true })
const file = path.join(dir, 'small_edges.json')
fs.writeFileSync(file, JSON.stringify({ note: 'tools/fixtures/make_local_small_edges.js: hand-shaped change requests, each encoded by the reference\'s encodeChange', entries }))
for (const e of entries) console.log(e.name, Buffer.from(e.change, 'base64').length, 'bytes')
console.log(file, fs.statSync(file).size, 'bytes')
