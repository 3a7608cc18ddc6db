// The sdmoe_tune knobs: ids (ABI, include/sdmoe.h defines every value) and the accessor the launch code reads them
// through. The table of names, defaults and legal values, the values themselves and sdmoe_tune live in tune.hip.
#pragma once

enum Knob {
  KNOB_STAGES = 0,
  KNOB_TILE = 1,
  KNOB_ATTN = 4,
  KNOB_DIAG = 6,
  KNOB_GN_FUSED = 7,
  KNOB_RES16 = 8,
  KNOB_KSPLIT = 9,
  KNOB_MFAST = 14,
  KNOB_TOPK = 15,
  KNOB_HALO = 16,
  KNOB_GT320 = 20,
  KNOB_NARROW = 21,
  KNOB_EPI_DIRECT = 23,
  KNOB_IDS = 24,  // one past the largest id
};

// current values by id (ids without a knob stay 0), in a struct so that tune.hip can constant-initialise them from the
// table's defaults; hidden: a pc-relative load like a file-local global, no GOT entry
struct KnobValues { int v[KNOB_IDS]; };
extern __attribute__((visibility("hidden"))) KnobValues sdmoe_knob_values;

inline int knob(int id) { return sdmoe_knob_values.v[id]; }
