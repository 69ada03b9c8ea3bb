// TEST INFRASTRUCTURE - the `-trans` parser (veryfasttree_amd/host/ReadTransition.h) as a stand-alone program, built and run by
// tests/test_distopt_cpu.py, with -fsanitize=address,undefined when asked; needs nothing but a C++11 compiler.
//   read_transition_check file ...
// Per file one line: `file <name> ok <sum of the 400 rates> <sum of the 20 frequencies>` (%.17g) or `file <name> refused (<message>)`.
// The text is handed over in a buffer of exactly its length, so that a read beyond it is a read beyond an allocation.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "../../veryfasttree_amd/host/ReadTransition.h"

int main(int argc, char **argv) {
    int unread = 0;
    for (int k = 1; k < argc; k++) {
        std::ifstream in(argv[k], std::ios::binary);
        if (!in) {
            printf("file %s cannot be read\n", argv[k]);
            unread++;
            continue;
        }
        const std::string bytes((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
        std::vector<char> exact(bytes.begin(), bytes.end());   // no terminator behind the text
        const char *name = strrchr(argv[k], '/') ? strrchr(argv[k], '/') + 1 : argv[k];
        double matrix[20][20], stat[20];
        try {
            veryfasttree::readAATransition(exact.data(), exact.size(), matrix, stat);
            double m = 0, s = 0;
            for (int i = 0; i < 20; i++) {
                s += stat[i];
                for (int j = 0; j < 20; j++) m += matrix[i][j];
            }
            printf("file %s ok %.17g %.17g\n", name, m, s);
        } catch (const std::exception &e) {
            printf("file %s refused (%s)\n", name, e.what());
        }
    }
    printf("unread %d\n", unread);
    return unread ? 1 : 0;
}
