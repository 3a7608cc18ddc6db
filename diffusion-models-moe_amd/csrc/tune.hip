// The one table of sdmoe_tune knobs (host only, no HIP call): id, name, default and legal values of each, the current
// values (tune.h: knob()), and the entry points that set, enumerate and reset them. What each value means is defined in
// include/sdmoe.h; why a default is what it is stands at the code the knob steers.
#include <cstdint>

#include "common.h"
#include "tune.h"
#include "../../include/sdmoe.h"

namespace {

struct KnobRow {
  int id;
  const char* name;
  int def;
  uint64_t legal;  // bit v set = value v accepted
};

constexpr uint64_t upto(int hi) { return hi >= 63 ? ~0ull : (1ull << (hi + 1)) - 1; }  // 0..hi
template <typename... V>
constexpr uint64_t anyof(V... v) { return ((1ull << v) | ...); }

constexpr KnobRow kKnobs[] = {
    {KNOB_STAGES, "stages", 0, anyof(0, 2, 3)},
    {KNOB_TILE, "tile", 0, upto(8)},
    {KNOB_ATTN, "attn", 0, anyof(0, 1, 2, 4, 8, 9)},
    {KNOB_DIAG, "diag", 0, upto(63)},
    {KNOB_GN_FUSED, "gn_fused", 1, upto(2)},
    {KNOB_RES16, "res16", 1, upto(1)},
    {KNOB_KSPLIT, "ksplit", 0, upto(32)},
    {KNOB_MFAST, "mfast", 1, upto(1)},
    {KNOB_TOPK, "topk", 0, anyof(0, 1, 4)},
    {KNOB_HALO, "halo", 1, upto(3)},
    {KNOB_GT320, "gt320", 1, upto(1)},
    {KNOB_NARROW, "narrow", 1, upto(1)},
    {KNOB_EPI_DIRECT, "epi_direct", 1, upto(2)},
};
constexpr int kNumKnobs = sizeof(kKnobs) / sizeof(kKnobs[0]);

constexpr KnobValues defaults() {
  KnobValues d{};
  for (const KnobRow& r : kKnobs) d.v[r.id] = r.def;
  return d;
}

}  // namespace

KnobValues sdmoe_knob_values = defaults();

extern "C" int sdmoe_tune(int knob, int value) {
  for (const KnobRow& r : kKnobs)
    if (r.id == knob && value >= 0 && value < 64 && (r.legal >> value & 1)) {
      sdmoe_knob_values.v[knob] = value;
      return SDMOE_OK;
    }
  return SDMOE_EARG;
}

extern "C" int sdmoe_tune_knob(int index, int* id, const char** name, int* default_value, int* value) {
  if (index < 0 || index >= kNumKnobs || !id || !name || !default_value || !value) return SDMOE_EARG;
  const KnobRow& r = kKnobs[index];
  *id = r.id; *name = r.name; *default_value = r.def; *value = sdmoe_knob_values.v[r.id];
  return SDMOE_OK;
}

extern "C" int sdmoe_tune_reset(void) {
  sdmoe_knob_values = defaults();
  return SDMOE_OK;
}
