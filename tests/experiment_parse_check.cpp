// Stand-alone check of parse_experiment (vdm4cdm_amd/csrc/experiment.h), built with AddressSanitizer + UBSan and run by
// tests/test_experiment_cpu.py: the strings of the Python parser's test, and strings the lenient parser must skip without harm.
#include <cstdio>
#include <string>

#include "../vdm4cdm_amd/csrc/experiment.h"

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

static bool all_default(const Experiment& e) {
#define X(key, dflt) if (e.key != dflt) return false;
    VDM_EXPERIMENT_KEYS(X)
#undef X
    return true;
}

static Experiment parsed(const char* text) { Experiment e; parse_experiment(text, e); return e; }

int main() {
    CHECK(all_default(Experiment{}));
    CHECK(all_default(parsed(nullptr)) && all_default(parsed("")) && all_default(parsed(" , ,,\t, ")));
    Experiment e = parsed("split=0, ksplit=0,wgrad_wgs=256,ablate=wgrad+conv1,grouped_reduce");
    CHECK(e.split == 0 && e.ksplit == 0 && e.wgrad_wgs == 256 && e.grouped_reduce == 1);
    CHECK(e.kpack == 1 && e.roll == 1 && e.thin_wgrad == 1 && e.wgrad_rows == 1 && e.wgrad_roll == 1 && e.ablate_reduce == 0);
    // keys of the Python side, a trailing comma, blanks around key and value
    e = parsed("fused_gn=0,fused_head=0,defer_wgrad_levels=2,ablate=pack, roll = 0 ,");
    CHECK(e.roll == 0);
    e.roll = 1;
    CHECK(all_default(e));
    // items it cannot read are skipped, the readable ones around them still count
    e = parsed("split=,ksplit=x,kpack=-1,roll=0x0,thin_wgrad=1 1,wgrad_wgs=99999999999,=0,split2=0,spli=0,wgrad_rows=0=0,ablate_reduce");
    CHECK(e.ablate_reduce == 1);
    e.ablate_reduce = 0;
    CHECK(all_default(e));
    CHECK(parsed("wgrad_wgs=999999999").wgrad_wgs == 999999999 && parsed("wgrad_wgs=007").wgrad_wgs == 7);
    CHECK(parsed("split=0,split=1").split == 1);      // (Python refuses a key given twice; here the last one holds)
    // 4 KiB of garbage, with and without separators in it
    std::string junk;
    for (int i = 0; i < 4096; ++i) junk += (char)(1 + (i * 131 + i / 7) % 255);
    CHECK(all_default(parsed(junk.c_str())));
    CHECK(all_default(parsed(std::string(4096, '=').c_str())) && all_default(parsed(std::string(4096, ',').c_str())));
    CHECK(parsed((std::string(4096, 'k') + ",kpack=0").c_str()).kpack == 0);
    if (!failures) puts("experiment parser ok");
    return failures != 0;
}
