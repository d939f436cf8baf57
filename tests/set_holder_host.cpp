// Stand-alone host program over br_amd/csrc/brx_setstate.hpp: prints who holds the keys of a set for the cases on its
// command line, one line per case.  Built and run by test_set_holder_cpu.py with -fsanitize=address,undefined; the
// expected lines are written out there.
//
//   SPARSE,STALE,LIST_VALID,LISTED_N,LIST_CAP,IDX_VALID,IDX_EXACT,HAVE_LINES
#include "../br_amd/csrc/brx_setstate.hpp"

#include <stdio.h>

using namespace brx;

static const char *const NAMES[4] = {"KeyList", "Table", "Bits", "None"}; // (in the enum's order)

int main(int argc, char **argv)
{
    for (int i = 1; i < argc; i++) {
        unsigned long long v[8];
        if (sscanf(argv[i], "%llu,%llu,%llu,%llu,%llu,%llu,%llu,%llu", v, v + 1, v + 2, v + 3, v + 4, v + 5, v + 6, v + 7) != 8) {
            fprintf(stderr, "bad case: %s\n", argv[i]);
            return 1;
        }
        puts(NAMES[(int)set_holder(v[0] != 0, v[1] != 0, v[2] != 0, v[3], v[4], v[5] != 0, v[6] != 0, v[7] != 0)]);
    }
    return 0;
}
