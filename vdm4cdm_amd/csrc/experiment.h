// The library's share of VDM4CDM_EXPERIMENT: a comma-separated list of `key` or `key=value` items (a bare key means key=1), the A/B and
// ablation switches of kernels.  Host code only; no HIP header.
//
// This parser is LENIENT: it skips keys it does not own (the Python-side ones) and items it cannot read.  The strict parser, which
// refuses unknown keys, repeated keys and values out of range, is vdm4cdm_amd/_experiment.py; it runs before the library is loaded.
#pragma once
#include <cstdlib>
#include <cstring>

// X(key, default): the same rows as the library keys of TABLE in _experiment.py (tests/test_experiment_cpu.py compares the two)
#define VDM_EXPERIMENT_KEYS(X)                                                                                                   \
    X(split, 1)          /* half-chunk workgroups of the NC=4 convs on small grids (conv_common.h uses_split) */                \
    X(ksplit, 1)         /* K-split kernel of the deepest levels (uses_ksplit) */                                                \
    X(kpack, 1)          /* tap-packed kernel of conv_in / conv_out */                                                           \
    X(roll, 1)           /* rolling-z forward / dgrad kernel: one K-block, large grid, persistent walk up z */                  \
    X(thin_wgrad, 1)     /* thin-side weight gradient of conv_in / conv_out (wgrad_thin.hip) */                                  \
    X(wgrad_rows, 1)     /* 0: the tap-split kernel also for the full bf16 3^3 stride-1 blocks */                                \
    X(wgrad_roll, 1)     /* 0: no rolling z window - the workgroups of the rows kernel walk scattered tiles, not column segments */ \
    X(wgrad_wgs, 512)    /* persistent workgroups of a weight-gradient launch over all (cout, cin) block pairs (~2 per CU) */   \
    X(grouped_reduce, 0) /* the grouped slab reduce also for few slabs (same result, other launch shape) */                      \
    X(ablate_reduce, 0)  /* timing ablation: the slab reduce is NOT launched - weight gradients are garbage */

struct Experiment {
#define X(key, dflt) int key = dflt;
    VDM_EXPERIMENT_KEYS(X)
#undef X
};

// Pure: fields named in `text` (may be null) are set, everything else is left as it is.  Values are non-negative decimal integers of at
// most 9 digits; blanks around items, keys and values are ignored.
inline void parse_experiment(const char* text, Experiment& e) {
    const auto blank = [](char c) { return c == ' ' || c == '\t'; };
    for (const char* p = text; p && *p;) {
        const char* end = strchr(p, ',');
        if (!end) end = p + strlen(p);
        const char* eq = (const char*)memchr(p, '=', end - p);
        const char *k0 = p, *k1 = eq ? eq : end;                 // key
        while (k0 < k1 && blank(*k0)) ++k0;
        while (k1 > k0 && blank(k1[-1])) --k1;
        int value = 1;
        bool ok = k1 > k0;
        if (eq) {
            const char *v0 = eq + 1, *v1 = end;
            while (v0 < v1 && blank(*v0)) ++v0;
            while (v1 > v0 && blank(v1[-1])) --v1;
            ok = ok && v1 > v0 && v1 - v0 <= 9;
            value = 0;
            for (const char* c = v0; ok && c < v1; ++c) {
                ok = *c >= '0' && *c <= '9';
                value = value * 10 + (*c - '0');
            }
        }
        const size_t len = k1 - k0;
#define X(key, dflt) if (ok && len == sizeof(#key) - 1 && !memcmp(k0, #key, len)) e.key = value;
        VDM_EXPERIMENT_KEYS(X)
#undef X
        p = *end ? end + 1 : end;
    }
}

// The process's switches: VDM4CDM_EXPERIMENT is read once (an inline function's local static: one instance for the whole shared object).
inline const Experiment& experiment() {
    static const Experiment e = [] { Experiment x; parse_experiment(getenv("VDM4CDM_EXPERIMENT"), x); return x; }();
    return e;
}
