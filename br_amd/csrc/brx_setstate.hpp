// Who holds the keys of a solid set right now: the one rule, on plain values (no HIP types: tests/set_holder_host.cpp
// compiles it with g++).  brx_set (brx_internal.hpp) can hold its keys four ways at once -- a current bit vector, a key
// list that may be truncated, a chained table that is exact on its own, an index that only accelerates the bits -- and
// every entry that enumerates or counts the keys asks set_keys (brx_index.hip), which reads the list's counter and asks
// this.
#pragma once
#include <stdint.h>

namespace brx {

enum class SetHolder { KeyList, Table, Bits, None };

// 1. A valid list that holds all it was given is the set (cheapest to read, and a lazy or sparse set may have nothing
//    else).  A truncated list (more keys found than it has room for) is no list: stated here and nowhere else.
// 2. Without a bit vector (sparse) or without a written one (lazy), only a table built with chaining holds every key.
//    If there is none the keys are nowhere: None.  Each caller has its own message for that.
// 3. Otherwise the bit vector.
inline SetHolder set_holder(bool sparse, bool bits_stale, bool keylist_valid, uint64_t listed_n, uint64_t list_cap, bool idx_valid,
                            bool idx_exact, bool have_lines)
{
    if (keylist_valid && listed_n <= list_cap)
        return SetHolder::KeyList;
    if (sparse || bits_stale)
        return idx_valid && idx_exact && have_lines ? SetHolder::Table : SetHolder::None;
    return SetHolder::Bits;
}

} // namespace brx
