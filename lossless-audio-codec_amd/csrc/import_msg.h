// import_msg.h -- host only: the outcome of an item's validation by the import pass (ImportBad, import_core.h) as the
// encoder words it.  All of left first, then right (the reference's order: check_sample_range, ref lac/encoder.cpp:82-102).
// Shared by api_import.cpp and the CPU twin (tests/native/sim_import.cpp).
#pragma once
#include <string>

#include "import_core.h"

namespace lacx {

// False: the item is clean.  True: *channel / *index say where, msg what ("left sample at index I is ...").
inline bool import_bad_message(const ImportBad& b, int bit_depth, int* channel, unsigned long long* index, std::string& msg) {
    const int ch = b.key[0] != kImportClean ? 0 : (b.key[1] != kImportClean ? 1 : -1);
    if (ch < 0) return false;
    *channel = ch;
    *index = b.key[ch] >> 1;
    msg = std::string(ch ? "right" : "left") + " sample at index " + std::to_string(*index);
    if (b.key[ch] & 1u) msg += " is not an exact " + std::to_string(bit_depth) + "-bit PCM value";
    else msg += " is outside the configured PCM bit depth";
    return true;
}

}  // namespace lacx
