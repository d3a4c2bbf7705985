// knobs.inc — the index's tuning knobs, said once (included by handles.inc, for sg_index): the table below is what the environment at the first
// upload, sg_index_tune(), sg_debug_knob() and DESIGN.md §4c all go by.  Results never depend on the knobs; tests sweep them.
// A row's flags: read from the environment at the first upload / may be set through sg_index_tune(); setting it pins the stream
// workgroup (takes pipe_shape_auto away); tune_choice() chooses it unless it was set explicitly; powers of two only.
enum : uint32_t { KNOB_ENV = 1u, KNOB_TUNE = 2u, KNOB_BOTH = KNOB_ENV | KNOB_TUNE, KNOB_SHAPE = 4u, KNOB_TUNER = 8u, KNOB_POW2 = 16u };

struct Knobs {
  int32_t log2_cnt, t_floor, filter_level, tighten, roomy, order, pretok, split_chunks, parts_cnt_bonus, g8;
  int32_t pipe, pipe_nw, pipe_log2_cnt, pipe_dt_bytes, pipe_shape_auto, pipe_shape_bias, pipe_sub, pipe_cand_cap, pipe_wide, plan2;
  uint32_t explicit_set = 0;   // bit i: row i came from the environment or sg_index_tune(), not from its default or the tuner
  Knobs();                     // every row's default
};
struct KnobRow { const char* name; int32_t Knobs::*field; int32_t lo, hi, def; uint32_t flags; const char* meaning; };

const KnobRow kKnobs[] = {
    {"SG_LOG2_CNT", &Knobs::log2_cnt, 9, 14, 11, KNOB_BOTH | KNOB_TUNER, "log2 of the LDS counter words per wavefront"},
    {"SG_T_FLOOR", &Knobs::t_floor, 2, 64, 8, KNOB_BOTH, "lowest flag threshold list skipping may leave"},
    {"SG_FILTER_LEVEL", &Knobs::filter_level, 0, 7, 4, KNOB_BOTH | KNOB_TUNER, "row of kBucketsPer16Postings: 0..3 strict, 4..7 loose"},
    {"SG_TIGHTEN", &Knobs::tighten, 0, 2, 2, KNOB_BOTH, "threshold tightening: 0 never, 1 always, 2 by the share of queries whose top-k fills"},
    {"SG_ROOMY", &Knobs::roomy, 0, 2, 2, KNOB_BOTH, "candidate queue: 0 small (12 wavefronts per CU), 1 large (11), 2 large for tightening and docID-ordered launches"},
    {"SG_ORDER", &Knobs::order, 0, INT32_MAX, 1, KNOB_BOTH, "heaviest queries first (query_order_kernel): 0 never, 1 batches of >= 8192, n >= 2: batches of >= n"},
    {"SG_PRETOK", &Knobs::pretok, 0, INT32_MAX, 2048, KNOB_BOTH, "batches of >= n queries are tokenised by a launch of their own (sg_terms_kernel); 0 never"},
    {"SG_SPLIT_CHUNKS", &Knobs::split_chunks, 0, INT32_MAX, 65536, KNOB_BOTH, "fewest 16-byte chunks per part of a split query (1 MiB of postings); 0 never split"},
    {"SG_PARTS_CNT_BONUS", &Knobs::parts_cnt_bonus, 0, 3, 2, KNOB_BOTH, "log2 of the counter-array growth of the parts launch for small batches"},
    {"SG_G8", &Knobs::g8, 0, 2, 0, KNOB_ENV, "8-bit gaps for dense terms (packed_store.inc; the store is packed at the first upload): 0 never (the store shrinks by a third on bigram indexes, but its chunks are 81 % full and the launches follow the posting SLOTS: cfg 4 -26 %), 1 where they save chunks, 2 every term (tests)"},
    {"SG_PIPE", &Knobs::pipe, 0, 2, 2, KNOB_BOTH, "plan -> stream -> verify (pipeline.inc): 0 never, 1 whenever a launch is eligible, 2 where it pays and the guard lets it"},
    {"SG_PIPE_NW", &Knobs::pipe_nw, 2, 8, 8, KNOB_BOTH | KNOB_TUNER | KNOB_SHAPE | KNOB_POW2, "wavefronts of a stream workgroup: 2, 4 or 8"},
    {"SG_PIPE_LOG2_CNT", &Knobs::pipe_log2_cnt, 9, 13, 13, KNOB_BOTH | KNOB_TUNER | KNOB_SHAPE, "log2 of the u32 counters of a stream workgroup"},
    {"SG_PIPE_DT_BYTES", &Knobs::pipe_dt_bytes, 1024, 32768, 8192, KNOB_BOTH | KNOB_TUNER | KNOB_SHAPE, "LDS of a stream workgroup's sub-row descriptors: with the counters, the workgroups a CU holds"},
    {"SG_PIPE_SHAPE_AUTO", &Knobs::pipe_shape_auto, 1, 1, 1, KNOB_TUNE, "1: the stream workgroup is chosen per launch (pipe_shape_model); 0 once a shape knob was given: every launch takes the three"},
    {"SG_PIPE_SHAPE_BIAS", &Knobs::pipe_shape_bias, -2, 0, 0, KNOB_TUNE, "test hook: the model's shape lowered by this much — a launch that starts too light"},
    {"SG_PIPE_SUB", &Knobs::pipe_sub, 3, 5, 4, KNOB_BOTH, "log2 of the chunks a row descriptor covers"},
    {"SG_PIPE_CAND_CAP", &Knobs::pipe_cand_cap, 1, 4096, 64, KNOB_BOTH, "candidate slots per query"},
    {"SG_PIPE_WIDE", &Knobs::pipe_wide, 0, 1, 0, KNOB_BOTH, "1: 8-byte sub-row descriptors whatever the store's size (tests; stores of 2^26 chunks and more take them anyway)"},
    {"SG_PLAN2", &Knobs::plan2, 0, 1, 1, KNOB_BOTH, "1: the plan launch with two queries per wavefront (plan2.inc) where the description allows it; 0: sg_plan_kernel alone"},
};
constexpr uint32_t kNumKnobs = sizeof kKnobs / sizeof kKnobs[0];
static_assert(kNumKnobs <= 32, "Knobs::explicit_set is 32 bits");
inline Knobs::Knobs() { for (const KnobRow& row : kKnobs) this->*row.field = row.def; }

inline bool knob_is_explicit(const Knobs& k, int32_t Knobs::*field) {
  for (uint32_t i = 0; i < kNumKnobs; i++) if (kKnobs[i].field == field) return (k.explicit_set >> i) & 1u;
  return false;
}
inline int knob_refused(const KnobRow& row, const std::string& why) {   // why + the range: "SG_PIPE_NW=3: out of range (2 .. 8, powers of two)"
  set_error(row.name + why + " (" + std::to_string(row.lo) + " .. " + std::to_string(row.hi) + (row.flags & KNOB_POW2 ? ", powers of two)" : ")"));
  return SG_E_INVALID;
}

// The one way a value from outside reaches a knob (source: KNOB_ENV or KNOB_TUNE): in range or SG_E_INVALID, no clamping.
inline int set_knob(Knobs& k, const KnobRow& row, int32_t value, uint32_t source) {
  if (!(row.flags & source)) return knob_refused(row, source == KNOB_ENV ? " is set through sg_index_tune only, not from the environment" : " is read from the environment at the first upload only, not set through sg_index_tune");
  if (value < row.lo || value > row.hi || ((row.flags & KNOB_POW2) && (value & (value - 1)))) return knob_refused(row, "=" + std::to_string(value) + ": out of range");
  k.*row.field = value; k.explicit_set |= 1u << (uint32_t)(&row - kKnobs);
  if (row.flags & KNOB_SHAPE) k.pipe_shape_auto = 0;
  return SG_OK;
}
