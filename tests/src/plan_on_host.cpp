// plan_on_host.cpp -- csrc/hmpc_plan.h on the CPU (tests/test_plan_on_host.py): which variant a batch runs on, the size-class launches,
// which status words are repaired, and which derived results are still valid, each against a restatement written here.
#include <stdio.h>

#include <map>
#include <tuple>
#include <vector>

#include "hmpc_plan.h"

static int problems = 0;
#define CHECK(cond, ...)                       \
  do {                                         \
    if (!(cond)) {                             \
      ++problems;                              \
      printf("FAILED %s: ", #cond);            \
      printf(__VA_ARGS__);                     \
      printf("\n");                            \
    }                                          \
  } while (0)

// The variant table from HMPC_VARIANT_TABLE's shapes, no kernels.  smem: any values that increase with NMAX and with HMAX -- that
// ordering is all pick_variant may rely on (the real footprints are sizeof(VariantTraits::SM), known only to the kernel's translation
// units).  Two assignments that order the incomparable pair <60,20> / <120,10> both ways.
static std::vector<Variant> table(int w_nmax, int w_hmax) {
#define ROW(IDX, GRP, NMAX, HMAX, NT, QCAP, NC, BPT, ROLE) \
  Variant{NMAX, HMAX, NT, QCAP, NC, Role::ROLE, false, nullptr, nullptr, (size_t)(w_nmax * NMAX + w_hmax * HMAX), 0, 0},
  return {HMPC_VARIANT_TABLE(ROW)};
#undef ROW
}

// pick_variant as the search it was before the map (fast_variant) was written down: of the two-contact fast variants that hold the
// horizon and the widest QP, the one with the smallest LDS footprint
static int pick_by_search(const std::vector<Variant> &v, int nc, int hz, int max_stance) {
  if (nc == 3) return 6;
  if (max_stance > 120 && hz > 10) return 8;
  int best = -1;
  for (int i = 0; i < 4; ++i) {
    if (v[i].hmax < hz) continue;
    if (max_stance >= 0 && v[i].nmax < max_stance) continue;
    if (max_stance < 0 && v[i].nmax < 120) continue;
    if (best < 0 || v[i].smem < v[best].smem) best = i;
  }
  return best < 0 ? 3 : best;
}

static void check_variants() {
  const std::vector<Variant> ta = table(64, 1), tb = table(1, 64);
  CHECK((int)ta.size() == N_VARIANTS, "%zu rows", ta.size());
  CHECK(ta[0].smem < ta[2].smem && ta[2].smem < ta[1].smem && tb[1].smem < tb[2].smem, "the two smem orders");
  const int stances[] = {-1, 0, 6, 54, 60, 66, 120, 126, 240, 246, 1000};
  for (int nc = 2; nc <= 3; ++nc)
    for (int hz = 1; hz <= 20; ++hz)
      for (int ms : stances) {
        int want;
        if (nc == 3) want = 6;
        else if (hz > 10 && ms > 120) want = 8;
        else {
          const int need = ms < 0 ? 120 : ms;
          if (hz <= 10) want = need <= 60 ? 0 : (need <= 120 ? 1 : 3);  // (3: the fallback for an oversize batch, reported per instance)
          else want = need <= 60 ? 2 : 3;
        }
        const int got = pick_variant(nc, hz, ms);
        CHECK(got == want, "pick_variant(%d, %d, %d) = %d, want %d", nc, hz, ms, got, want);
        CHECK(got == pick_by_search(ta, nc, hz, ms) && got == pick_by_search(tb, nc, hz, ms), "pick_variant(%d, %d, %d) = %d against the search",
              nc, hz, ms, got);
        if (nc == 2 && got < N_FAST) CHECK(ta[got].hmax >= (hz > 10 ? 20 : 10) && ta[got].role == Role::FAST, "variant %d holds h = %d", got, hz);
        for (int ult = 0; ult < 2; ++ult) {
          CHECK(repair_variant(Role::CONT, nc, hz, ms, ult) == 11 + (hz > 10), "CONT(%d, %d, %d)", nc, hz, ms);
          const int safe = repair_variant(Role::SAFE, nc, hz, ms, ult);
          const int want_safe = want == 8 ? 9 : (nc == 3 ? (ult ? 10 : 7) : 4 + (hz > 10));
          CHECK(safe == want_safe, "SAFE(%d, %d, %d, %d) = %d, want %d", nc, hz, ms, ult, safe, want_safe);
          if (nc == 2 || hz <= 10)  // (a three-contact handle exists for h <= 10 only)
            CHECK(ta[safe].role == Role::SAFE && ta[safe].nmax >= ta[got].nmax && ta[safe].hmax >= hz, "SAFE variant %d behind %d at h = %d", safe, got, hz);
        }
      }
}

static void check_class_tables() {
  struct Want {
    bool sweep, long_h;
    int n;
    ClassLaunch l[3];
  };
  const Want wants[] = {{false, false, 2, {{0, 0, 10}, {1, 11, 255}}},
                        {false, true, 3, {{2, 0, 10}, {3, 11, 20}, {8, 21, 255}}},
                        {true, false, 2, {{14, 0, 10}, {13, 11, 255}}}};
  for (const Want &w : wants) {
    ClassLaunch l[SIZE_CLASSES] = {};
    const int n = class_launches(w.sweep, w.long_h, l);
    CHECK(n == w.n, "class_launches(%d, %d) = %d launches", w.sweep, w.long_h, n);
    for (int k = 0; k < w.n && k < n; ++k)
      CHECK(l[k].vi == w.l[k].vi && l[k].lo == w.l[k].lo && l[k].hi == w.l[k].hi, "class_launches(%d, %d)[%d] = {%d, [%d, %d]}", w.sweep,
            w.long_h, k, l[k].vi, l[k].lo, l[k].hi);
  }
  // a class byte is a count of stance leg-steps, six reduced variables each: the classes are the size classes pick_variant sorts by
  for (int steps = 0; steps <= 40; ++steps) {
    ClassLaunch l[SIZE_CLASSES];
    const int n = class_launches(false, true, l);
    int hit = -1;
    for (int k = 0; k < n; ++k)
      if (l[k].lo <= steps && steps <= l[k].hi) {
        CHECK(hit < 0, "%d leg-steps in two classes", steps);
        hit = l[k].vi;
      }
    CHECK(hit == pick_variant(2, 20, 6 * steps), "%d leg-steps: class launch %d, pick_variant %d", steps, hit, pick_variant(2, 20, 6 * steps));
  }
  CHECK(flag_list_cap(100) == 100 && flag_list_cap(1 << 20) == REPAIR_GRID_CAP, "flag_list_cap");
  CHECK(device_list_len(100, false) == 100 && device_list_len(1 << 20, false) == REPAIR_GRID_CAP && device_list_len(100, true) == 100 &&
            device_list_len(5000, true) == REPAIR_GRID_CAP_WIDE,
        "device_list_len");
  CHECK(reg_list_len(8) == 8 && reg_list_len(8192) == REG_LIST_CAP, "reg_list_len");
  // batch 600 is the smallest round size with a dispatch order; none for single-support batches, external QPs, mode 0, without buffers
  CHECK(!orders_dispatch(1, true, 512, 2, 120, false) && orders_dispatch(1, true, 513, 2, 120, false) && orders_dispatch(2, true, 32768, 2, -1, false) &&
            !orders_dispatch(1, true, 32769, 2, 120, false) && !orders_dispatch(1, true, 600, 2, 60, false) && orders_dispatch(1, true, 600, 3, 60, false) &&
            !orders_dispatch(0, true, 600, 2, 120, false) && !orders_dispatch(1, false, 600, 2, 120, false) && !orders_dispatch(1, true, 600, 2, 120, true),
        "orders_dispatch");
}

// The three expressions as they stood where they were written out by hand: the list of hmpc_resolve_failed, its relaxed passes, and the
// legacy tick's test of the fast launch's status word.
static bool old_capped(int iter_cap, uint32_t status) {
  return iter_cap > 0 && (int)HMPC_STATUS_ITERS(status) >= iter_cap && (int)HMPC_STATUS_ITERS(status) <= iter_cap + 1;
}
static bool old_resolve_list(uint32_t w, int cap) {
  const uint32_t c = HMPC_STATUS_CODE(w);
  return c == HMPC_S_WORKSET || (c == HMPC_S_MAXITER && !old_capped(cap, w)) || c == HMPC_S_INFEASIBLE || c == HMPC_S_KKT || c == HMPC_S_INDEFINITE;
}
static bool old_relaxed_pass(uint32_t w, int cap) {
  const uint32_t c = HMPC_STATUS_CODE(w);
  return (c == HMPC_S_MAXITER && !old_capped(cap, w)) || c == HMPC_S_INFEASIBLE || c == HMPC_S_KKT || c == HMPC_S_WORKSET;
}
static bool old_legacy_tick(uint32_t w, int cap) {
  const uint32_t c0 = HMPC_STATUS_CODE(w);
  return c0 == HMPC_S_WORKSET || (c0 == HMPC_S_MAXITER && !old_capped(cap, w)) || c0 == HMPC_S_INFEASIBLE || c0 == HMPC_S_KKT;
}

static void check_predicates() {
  for (uint32_t code = 0; code <= 9; ++code)
    for (int cap : {0, 5})
      for (uint32_t iters : {4u, 5u, 6u, 7u}) {
        const uint32_t w = code | (iters << 8);
        CHECK(capped_by_caller(cap, w) == (cap == 5 && (iters == 5 || iters == 6)), "capped_by_caller(%d, code %u iters %u)", cap, code, iters);
        CHECK(needs_repair(w, cap) == old_resolve_list(w, cap), "needs_repair(code %u iters %u, cap %d)", code, iters, cap);
        CHECK(flagged(w, cap) == old_relaxed_pass(w, cap), "flagged(code %u iters %u, cap %d) against the relaxed passes", code, iters, cap);
        CHECK(flagged(w, cap) == old_legacy_tick(w, cap), "flagged(code %u iters %u, cap %d) against the legacy tick", code, iters, cap);
        CHECK(needs_repair(w, cap) == (flagged(w, cap) || code == HMPC_S_INDEFINITE), "needs_repair = flagged or indefinite (code %u)", code);
      }
}

// ResultState against the rules: batch -> solve -> prediction -> selection, solve -> margins; whatever replaces a node makes everything
// behind it stale; moving a result's buffers makes it and what was derived from it stale.  An entry point asks before it derives
// (`needs`), so only those transitions are applied.
enum : int { SOLVE = 1, PRED = 2, SEL = 4, MAR = 8 };
struct Rule {
  const char *name;
  int needs, sets, clears, groups;
  void (*apply)(ResultState &);
};
static const Rule RULES[] = {
    {"on_batch", 0, 0, SOLVE | PRED | SEL | MAR, -1, [](ResultState &r) { r.on_batch(); }},
    {"on_solve", 0, SOLVE, PRED | SEL | MAR, -1, [](ResultState &r) { r.on_solve(); }},
    {"on_predict", SOLVE, PRED, SEL, -1, [](ResultState &r) { r.on_predict(); }},
    {"on_select(3)", PRED, SEL, 0, 3, [](ResultState &r) { r.on_select(3); }},
    {"on_select(5)", PRED, SEL, 0, 5, [](ResultState &r) { r.on_select(5); }},
    {"on_margins", SOLVE, MAR, 0, -1, [](ResultState &r) { r.on_margins(); }},
    {"retarget_prediction", 0, 0, PRED | SEL, -1, [](ResultState &r) { r.retarget_prediction(); }},
    {"retarget_selection", 0, 0, SEL, -1, [](ResultState &r) { r.retarget_selection(); }},
    {"retarget_margins", 0, 0, MAR, -1, [](ResultState &r) { r.retarget_margins(); }},
};
struct Model {
  int facts = 0, groups = 0;  // groups: of the last selection, reported only while it is valid
  bool operator<(const Model &o) const { return std::tie(facts, groups) < std::tie(o.facts, o.groups); }
};
static void compare(const ResultState &r, const Model &m, const char *how) {
  CHECK(r.has_solve() == !!(m.facts & SOLVE) && r.has_prediction() == !!(m.facts & PRED) && r.has_selection() == !!(m.facts & SEL) &&
            r.has_margins() == !!(m.facts & MAR) && r.selected_groups() == ((m.facts & SEL) ? m.groups : 0),
        "%s: solve %d prediction %d selection %d margins %d groups %d, model facts %d groups %d", how, r.has_solve(), r.has_prediction(),
        r.has_selection(), r.has_margins(), r.selected_groups(), m.facts, m.groups);
  CHECK((!r.has_selection() || r.has_prediction()) && (!r.has_prediction() || r.has_solve()) && (!r.has_margins() || r.has_solve()),
        "%s: a result without what it was derived from", how);
}

static void check_result_state() {
  std::map<Model, ResultState> seen;
  std::vector<Model> todo = {Model{}};
  seen[Model{}] = ResultState{};
  compare(seen[Model{}], Model{}, "a new handle");
  while (!todo.empty()) {
    const Model m = todo.back();
    todo.pop_back();
    for (const Rule &rule : RULES) {
      if ((m.facts & rule.needs) != rule.needs) continue;
      ResultState r = seen[m];
      rule.apply(r);
      Model n = m;
      n.facts = (m.facts & ~rule.clears) | rule.sets;
      if (rule.groups >= 0) n.groups = rule.groups;
      compare(r, n, rule.name);
      if (!seen.count(n)) seen[n] = r, todo.push_back(n);
    }
  }
  CHECK(seen.size() >= 12, "%zu states reached", seen.size());
  {  // prediction (and a selection, and margins) then solve -> prediction, selection and margins stale
    ResultState r;
    r.on_solve(), r.on_predict(), r.on_select(4), r.on_margins();
    CHECK(r.has_prediction() && r.has_selection() && r.has_margins() && r.selected_groups() == 4, "everything derived");
    r.on_solve();
    CHECK(r.has_solve() && !r.has_prediction() && !r.has_selection() && !r.has_margins() && r.selected_groups() == 0, "a later solve");
  }
  {  // retarget_prediction -> selection stale as well; margins are not derived from it
    ResultState r;
    r.on_solve(), r.on_predict(), r.on_select(4), r.on_margins();
    r.retarget_prediction();
    CHECK(r.has_solve() && !r.has_prediction() && !r.has_selection() && r.has_margins() && r.selected_groups() == 0, "retarget_prediction");
  }
  {  // a new batch -> everything stale, select_groups reported 0
    ResultState r;
    r.on_solve(), r.on_predict(), r.on_select(4), r.on_margins();
    r.on_batch();
    CHECK(!r.has_solve() && !r.has_prediction() && !r.has_selection() && !r.has_margins() && r.selected_groups() == 0, "a new batch");
  }
}

int main() {
  check_variants();
  check_class_tables();
  check_predicates();
  check_result_state();
  hmpc_params p = {9.0f, {0.5f, 0.5f, 0.07f}, 2.0f, 0.09f, 0.06f, 9.81f};
  CHECK(params_ok(p), "default-like parameters");
  p.mass = 0.0f;
  CHECK(!params_ok(p), "zero mass");
  printf("%d problems\n", problems);
  return problems ? 1 : 0;
}
