// Runs the simulator's cutting rules (mind_the_gaps_amd/csrc/mtg_sim_plan.h) on the host for tests/test_sim_plan_cpu.py:
// one case per line of standard input as key=value tokens, one line of decisions per case.
//   layout:  nfft=.. S=.. transform=.. pairs=.. [env=..]     S is a number, "max" (INT64_MAX: a full call) or
//            "full-1" / "full" / "full+1" around the series per execution of a full call
//   lru:     lru=1 want=n2,S,P slot0=have,n2,S,P,used slot1=.. slot2=.. slot3=..
#include "mtg_sim_plan.h"

#include <iostream>
#include <sstream>
#include <string>

namespace {

void fields(const std::string &v, long long *out, int n)
{
    std::istringstream in(v);
    std::string item;
    for (int i = 0; i < n && std::getline(in, item, ','); ++i) out[i] = std::stoll(item);
}

}  // namespace

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        long long nfft = 0, want[3] = {0, 0, 0};
        int transform = 0, pairs = 1, env = 0;
        bool lru = false;
        std::string S = "max";
        MtgAcfSlot slots[MTG_ACF_SLOTS] = {};
        std::istringstream tokens(line);
        std::string tok;
        while (tokens >> tok) {
            const size_t eq = tok.find('=');
            const std::string k = tok.substr(0, eq), v = tok.substr(eq + 1);
            if (k == "nfft") nfft = std::stoll(v);
            else if (k == "S") S = v;
            else if (k == "transform") transform = std::stoi(v);
            else if (k == "pairs") pairs = std::stoi(v);
            else if (k == "env") env = std::stoi(v);
            else if (k == "lru") lru = true;
            else if (k == "want") fields(v, want, 3);
            else if (k.compare(0, 4, "slot") == 0 && k.size() == 5 && k[4] >= '0' && k[4] < '0' + MTG_ACF_SLOTS) {
                long long f[5] = {0, 0, 0, 0, 0};
                fields(v, f, 5);
                slots[k[4] - '0'] = MtgAcfSlot{f[0] != 0, f[1], f[2], f[3], (uint64_t)f[4]};
            } else { std::cerr << "unknown key " << k << "\n"; return 2; }
        }
        if (lru) {
            bool hit = false;
            const int at = mtg_acf_slot_choose(slots, want[0], want[1], want[2], &hit);
            std::cout << "slot=" << at << " hit=" << hit << "\n";
            continue;
        }
        int64_t s = INT64_MAX;
        if (S.compare(0, 4, "full") == 0) {
            s = mtg_sim_layout(nfft, INT64_MAX, transform, pairs != 0, env).chunk;
            if (S.size() > 4) s += S[4] == '+' ? 1 : -1;
        } else if (S != "max") {
            s = std::stoll(S);
        }
        const MtgSimLayout l = mtg_sim_layout(nfft, s, transform, pairs != 0, env);
        std::cout << "S=" << s << " czt=" << l.czt << " m=" << l.m << " per=" << l.per << " batch=" << l.batch << " chunk=" << l.chunk
                  << " slot=" << l.slot << " spec=" << l.spec_bytes << " series=" << l.series_bytes << " work=" << l.work_bytes << "\n";
    }
    return 0;
}
