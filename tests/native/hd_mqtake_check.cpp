// hd_mqtake_check.cpp -- the locate of a delivered row's sender
// (hyperdrive_amd/csrc/hd_mqtake.h, the text k_mq_take_rows compiles) as a
// stand-alone host program, so that it runs as plain C++ under ASan + UBSan
// (tests/test_mqtake_host.py).
//
// stdin, any number of cases:
//   case <ns> <nk>
//   <off[0]> ... <off[ns-1]>        the plan's exclusive offsets
//   <k> ...                         nk delivered rows, each below the total
// stdout per case:
//   s <sender of row k> ...
#include <cstdio>
#include <iostream>
#include <string>
#include <vector>

#include "../../hyperdrive_amd/csrc/hd_mqtake.h"

int main() {
    std::string word;
    while (std::cin >> word) {
        if (word != "case") return 2;
        uint32_t ns, nk;
        if (!(std::cin >> ns >> nk) || ns == 0) return 2;
        // exact sizes, no slack: an index one past the table is ASan's to catch
        std::vector<uint32_t> off(ns), ks(nk);
        for (uint32_t s = 0; s < ns; s++)
            if (!(std::cin >> off[s])) return 2;
        for (uint32_t j = 0; j < nk; j++)
            if (!(std::cin >> ks[j])) return 2;
        printf("s");
        for (uint32_t j = 0; j < nk; j++) printf(" %u", hd::mq_take_locate(off.data(), ns, ks[j]));
        printf("\n");
    }
    return 0;
}
