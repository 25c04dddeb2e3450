// Host-side rendering of the patch IR as JSON text identical to JSON.stringify(Backend.getPatch(state)).
#pragma once
#include "../../include/am355.h"
#include <string>

namespace am355 {
// local: the envelope of a patch of am355_apply_local_change (actor and seq behind diffs), or null
bool render_patch_json(const am355_patch_ir& ir, std::string& out, std::string& err, const am355_local_envelope* local = nullptr);
}
