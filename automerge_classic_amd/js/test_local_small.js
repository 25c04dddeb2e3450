// Small local changes through the JS host: index.js switches am355_set_local_small on for every context it makes (unless
// MI355X_LOCAL_SMALL=0), so the change of every applyLocalChange call inside the path's limits is built by one workgroup (csrc/am355_hist.hip kl_small)
// instead of by the bulk encoders. The sessions of tests/golden/local/sessions.json go through the wrapper exactly as test_local_change.js
// runs them -- every returned binaryChange, patch and heads the recorded one, the rejected requests alone on the reference path -- and
// afterwards the contexts must report that the one workgroup built the changes, none of them beyond its limits.
//   MI355X_LOCAL_SMALL=1 AM355_LOCAL_SMALL_VERIFY=1 node automerge_classic_amd/js/test_local_small.js
'use strict'
const path = require('path')
const assert = require('assert')
assert.notStrictEqual(process.env.MI355X_LOCAL_SMALL, '0', 'run without MI355X_LOCAL_SMALL=0')
const Backend = require(path.join(__dirname, 'index.js'))
require(path.join(__dirname, 'test_local_change.js'))   // the sessions, call by call, with its own assertions (the same module instance of index.js)
const c = Backend._counters
const [small, bulk] = Backend._localSmallCalls()
assert.ok(small > 0 && small >= c.gpuApplyLocalChange, `changes built by the one workgroup: ${small} of ${c.gpuApplyLocalChange} served local calls`)
assert.strictEqual(bulk, 0, 'a recorded request lay outside the limits of the small path')
assert.strictEqual(c.localFallbacks, 3, 'localFallbacks counts the rejected requests only: ' + JSON.stringify(c))
console.log(JSON.stringify({ small, bulk, counters: c }))
console.log('small local changes through the JS host: ok')
