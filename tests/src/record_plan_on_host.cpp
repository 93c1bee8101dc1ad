// tests/test_record_plan_on_host.py: the record-gradient node of ResultState (csrc/hmpc_plan.h) on the CPU, beside
// tests/src/limit_plan_on_host.cpp (which covers its parents): solve -> adjoint -> (model gradients, limit gradients) -> record gradients.
// From every reachable state under every transition of the adjoint's branch the facts are compared with a model of the rules: record
// gradients can be enqueued only while all three parents stand (can_record_adjoint); they are valid after on_record_adjoint and stale
// after every batch, every solve, on_adjoint, on_model_adjoint, on_limit_adjoint (new inputs), the three parents' retargets and their
// own; nothing of this branch touches the prediction, the margins, the certificate or the gains.
#include "hmpc_plan.h"
#include <cstdio>
#include <map>
#include <vector>

static int bad = 0;
#define CHECK(cond, ...)                       \
  do {                                         \
    if (!(cond)) {                             \
      ++bad;                                   \
      printf("line %d: ", __LINE__);           \
      printf(__VA_ARGS__);                     \
      printf("\n");                            \
    }                                          \
  } while (0)

enum { SOLVE = 1, ADJ = 2, MODEL = 4, LIMIT = 8, RECORD = 16, MARGINS = 32 };
struct Move {
  const char *name;
  int sets, clears;
  void (*apply)(ResultState &);
};
static const Move MOVES[] = {
    {"on_batch", 0, SOLVE | ADJ | MODEL | LIMIT | RECORD | MARGINS, [](ResultState &r) { r.on_batch(); }},
    {"on_solve", SOLVE, ADJ | MODEL | LIMIT | RECORD | MARGINS, [](ResultState &r) { r.on_solve(); }},
    {"on_adjoint", ADJ, MODEL | LIMIT | RECORD, [](ResultState &r) { r.on_adjoint(); }},
    {"on_model_adjoint", MODEL, RECORD, [](ResultState &r) { r.on_model_adjoint(); }},
    {"on_limit_adjoint", LIMIT, RECORD, [](ResultState &r) { r.on_limit_adjoint(); }},
    {"on_record_adjoint", RECORD, 0, [](ResultState &r) { r.on_record_adjoint(); }},
    {"on_margins", MARGINS, 0, [](ResultState &r) { r.on_margins(); }},
    {"retarget_adjoint", 0, ADJ | MODEL | LIMIT | RECORD, [](ResultState &r) { r.retarget_adjoint(); }},
    {"retarget_model_adjoint", 0, MODEL | RECORD, [](ResultState &r) { r.retarget_model_adjoint(); }},
    {"retarget_limit_adjoint", 0, LIMIT | RECORD, [](ResultState &r) { r.retarget_limit_adjoint(); }},
    {"retarget_record_adjoint", 0, RECORD, [](ResultState &r) { r.retarget_record_adjoint(); }},
    {"retarget_margins", 0, MARGINS, [](ResultState &r) { r.retarget_margins(); }},
};
// the C entry points refuse a launch whose input is missing, so the walk only makes the moves they would make
static bool allowed(const Move &m, int facts) {
  if (m.sets == ADJ || m.sets == MARGINS) return facts & SOLVE;
  if (m.sets == MODEL || m.sets == LIMIT) return facts & ADJ;
  if (m.sets == RECORD) return (facts & (ADJ | MODEL | LIMIT)) == (ADJ | MODEL | LIMIT);
  return true;
}
static int facts_of(const ResultState &r) {
  return (r.has_solve() ? SOLVE : 0) | (r.has_adjoint() ? ADJ : 0) | (r.has_model_adjoint() ? MODEL : 0) | (r.has_limit_adjoint() ? LIMIT : 0) |
         (r.has_record_adjoint() ? RECORD : 0) | (r.has_margins() ? MARGINS : 0);
}

int main() {
  std::map<int, ResultState> seen;
  std::vector<int> todo{0};
  seen[0] = ResultState{};
  CHECK(facts_of(seen[0]) == 0 && !seen[0].can_record_adjoint(), "a new handle has results");
  while (!todo.empty()) {
    const int f = todo.back();
    todo.pop_back();
    CHECK(seen[f].can_record_adjoint() == ((f & (ADJ | MODEL | LIMIT)) == (ADJ | MODEL | LIMIT)), "can_record_adjoint in %d", f);
    for (const Move &m : MOVES) {
      if (!allowed(m, f)) continue;
      ResultState r = seen[f];
      m.apply(r);
      const int want = (f & ~m.clears) | m.sets, got = facts_of(r);
      CHECK(got == want, "%s from %d: %d, want %d", m.name, f, got, want);
      CHECK((!(got & RECORD) || (got & (ADJ | MODEL | LIMIT)) == (ADJ | MODEL | LIMIT)) && (!(got & LIMIT) || (got & ADJ)) && (!(got & MODEL) || (got & ADJ)) &&
                (!(got & ADJ) || (got & SOLVE)),
            "%s from %d: a result without its input", m.name, f);
      CHECK(!r.has_prediction() && !r.has_selection() && !r.has_certificate() && !r.has_gains() && !r.has_first_order(), "%s touched another branch", m.name);
      if (!seen.count(got)) seen[got] = r, todo.push_back(got);
    }
  }
  // nothing; a solve, x margins (2); an adjoint x model x limits x margins (8); all three and record gradients, x margins (2)
  CHECK(seen.size() == 13, "%zu states reached", seen.size());
  printf("%d problems\n", bad);
  return bad != 0;
}
