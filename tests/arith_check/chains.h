// chains.h -- the moduli under test: every chain on the command line ("N,L,t,q_0,..,q_{L-1},p_0,..,p_L", from tests/param_chains.py)
// goes through HostParams::init, and each distinct modulus of it (the plaintext modulus included) is tested with the Mod and
// the twiddles that init computed.
#pragma once
#include "check.h"

namespace ac {

static inline bool load_chain(const char *spec, std::vector<ModCase> &out)
{
    std::vector<u64> v;
    for (const char *p = spec; *p;) {
        char *e;
        v.push_back(strtoull(p, &e, 10));
        if (e == p) return false;
        p = *e == ',' ? e + 1 : e;
        if (*e && *e != ',') return false;
    }
    if (v.size() < 3 || v.size() != 3 + 2 * v[1] + 1) return false;
    const u32 N = (u32)v[0], L = (u32)v[1];
    piehip::HostParams hp;
    const std::string msg = hp.init(N, L, v[2], v.data() + 3, v.data() + 3 + L);
    if (!msg.empty()) {
        fprintf(stderr, "chain %s: %s\n", spec, msg.c_str());
        return false;
    }
    for (u32 a = 0; a <= hp.M; a++) {
        bool seen = false;
        for (const ModCase &mc : out) seen |= mc.m.q == hp.dc.mod[a].q;
        if (seen) continue;
        ModCase mc;
        mc.m = hp.dc.mod[a];
        mc.plaintext = a == hp.M;
        if (a < hp.M) {
            for (u32 k : {1u, 2u, 3u, N / 2, N / 2 + 1, N - 1}) {
                mc.tw.push_back(hp.tw[a][k]), mc.tw_sh.push_back(hp.tw_sh[a][k]);
                mc.tw.push_back(hp.itw[a][k]), mc.tw_sh.push_back(hp.itw_sh[a][k]);
            }
            mc.tw.push_back(mc.m.n_inv), mc.tw_sh.push_back(mc.m.n_inv_sh);
        }
        out.push_back(mc);
    }
    return true;
}

}  // namespace ac
