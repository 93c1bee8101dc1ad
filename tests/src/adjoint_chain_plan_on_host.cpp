// tests/test_adjoint_chain_plan_on_host.py: the chain's node of ResultState (csrc/hmpc_plan.h) on the CPU, beside
// tests/src/adjoint_multi_plan_on_host.cpp (which covers the branch without it): solve -> multi-seed adjoint -> chain.  From every
// reachable state under every transition of the branch -- batch, solve, single adjoint, multi-seed adjoint, selection, the three
// single-seed downstream launches, the chain and the retargets of the adjoint, the multi-seed adjoint, the model, limit and record
// gradients and the chain -- the facts are compared with a model of the rules: the chain stands behind a multi-seed adjoint alone; it goes
// stale on every batch, every solve, every new multi-seed launch, the multi-seed adjoint's retarget and its own; nothing else touches
// it, and it touches nothing else: with the chain's bit masked out every move leaves exactly the facts the rules without the chain give
// (the parent's model, restated from tests/src/adjoint_multi_plan_on_host.cpp), whatever the chain's state.
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

// SEL: the current adjoint is a selected slice (only with ADJ and MULTI)
enum { SOLVE = 1, ADJ = 2, MODEL = 4, LIMIT = 8, RECORD = 16, MULTI = 32, SEL = 64, CHAIN = 128 };
constexpr int DOWN = MODEL | LIMIT | RECORD, CURRENT = ADJ | DOWN | SEL;
constexpr int SEEDS = 5, SLICE = 3;

// what a move makes of the facts without the chain, by the parent's rules
static int parent_model(const char kind, const int f) {
  const int fall = (f & SEL) ? CURRENT : 0;  // a selection falls with what it points into
  switch (kind) {
    case 'b': return 0;                                     // on_batch
    case 's': return SOLVE;                                 // on_solve
    case 'a': return (f & ~(DOWN | SEL)) | ADJ;             // on_adjoint
    case 'm': return (f & ~RECORD) | MODEL;                 // on_model_adjoint
    case 'l': return (f & ~RECORD) | LIMIT;                 // on_limit_adjoint
    case 'r': return f | RECORD;                            // on_record_adjoint
    case 'M': return (f & ~fall) | MULTI;                   // on_adjoint_multi
    case 'S': return (f & ~DOWN) | ADJ | SEL;               // on_select_adjoint
    case 'A': return f & ~CURRENT;                          // retarget_adjoint
    case 'T': return f & ~fall & ~MULTI;                    // retarget_adjoint_multi
    case 'x': return f & ~(MODEL | RECORD);                 // retarget_model_adjoint
    case 'y': return f & ~(LIMIT | RECORD);                 // retarget_limit_adjoint
    case 'z': return f & ~RECORD;                           // retarget_record_adjoint
  }
  return -1;
}
// ... and with it
static int model(const char kind, const int f) {
  if (kind == 'C') return f | CHAIN;                                    // on_adjoint_chain
  if (kind == 'U') return f & ~CHAIN;                                   // retarget_adjoint_chain
  const int old = parent_model(kind, f & ~CHAIN);
  const bool falls = kind == 'b' || kind == 's' || kind == 'M' || kind == 'T';
  return old | (falls ? 0 : (f & CHAIN));
}
static void apply(const char kind, ResultState &r) {
  switch (kind) {
    case 'b': r.on_batch(); break;
    case 's': r.on_solve(); break;
    case 'a': r.on_adjoint(); break;
    case 'm': r.on_model_adjoint(); break;
    case 'l': r.on_limit_adjoint(); break;
    case 'r': r.on_record_adjoint(); break;
    case 'M': r.on_adjoint_multi(SEEDS); break;
    case 'S': r.on_select_adjoint(SLICE); break;
    case 'A': r.retarget_adjoint(); break;
    case 'T': r.retarget_adjoint_multi(); break;
    case 'x': r.retarget_model_adjoint(); break;
    case 'y': r.retarget_limit_adjoint(); break;
    case 'z': r.retarget_record_adjoint(); break;
    case 'C': r.on_adjoint_chain(); break;
    case 'U': r.retarget_adjoint_chain(); break;
  }
}
// the C entry points refuse a launch whose input is missing, so the walk only makes the moves they would make
static bool allowed(const char kind, const int f) {
  if (kind == 'a' || kind == 'M') return f & SOLVE;
  if (kind == 'S' || kind == 'C') return f & MULTI;
  if (kind == 'm' || kind == 'l') return f & ADJ;
  if (kind == 'r') return (f & (ADJ | MODEL | LIMIT)) == (ADJ | MODEL | LIMIT);
  return true;
}
static int facts_of(const ResultState &r) {
  return (r.has_solve() ? SOLVE : 0) | (r.has_adjoint() ? ADJ : 0) | (r.has_model_adjoint() ? MODEL : 0) | (r.has_limit_adjoint() ? LIMIT : 0) |
         (r.has_record_adjoint() ? RECORD : 0) | (r.has_adjoint_multi() ? MULTI : 0) | (r.selected_adjoint_seed() >= 0 ? SEL : 0) |
         (r.has_adjoint_chain() ? CHAIN : 0);
}

int main() {
  const char MOVES[] = "bsamlrMSATxyzCU";
  std::map<int, ResultState> seen;
  std::vector<int> todo{0};
  seen[0] = ResultState{};
  CHECK(facts_of(seen[0]) == 0 && seen[0].adjoint_multi_seeds_enqueued() == 0 && seen[0].selected_adjoint_seed() == -1, "a new handle has results");
  while (!todo.empty()) {
    const int f = todo.back();
    todo.pop_back();
    const ResultState &at = seen[f];
    CHECK(at.adjoint_multi_seeds_enqueued() == ((f & MULTI) ? SEEDS : 0), "the seeds in %d", f);
    CHECK(at.selected_adjoint_seed() == ((f & SEL) ? SLICE : -1), "the selected slice in %d", f);
    CHECK(at.can_record_adjoint() == ((f & (ADJ | MODEL | LIMIT)) == (ADJ | MODEL | LIMIT)), "can_record_adjoint in %d", f);
    for (const char *m = MOVES; *m; ++m) {
      if (!allowed(*m, f)) continue;
      ResultState r = seen[f];
      apply(*m, r);
      const int want = model(*m, f), got = facts_of(r);
      CHECK(got == want, "move %c from %d: %d, want %d", *m, f, got, want);
      if (*m != 'C' && *m != 'U') CHECK((got & ~CHAIN) == parent_model(*m, f & ~CHAIN), "move %c from %d: an accessor of the parent's answers %d", *m, f, got & ~CHAIN);
      else CHECK((got & ~CHAIN) == (f & ~CHAIN) && r.adjoint_multi_seeds_enqueued() == at.adjoint_multi_seeds_enqueued() && r.selected_adjoint_seed() == at.selected_adjoint_seed() && r.can_record_adjoint() == at.can_record_adjoint(), "move %c from %d touched another node", *m, f);
      CHECK(!(got & CHAIN) || (got & MULTI), "move %c from %d: a chain without its multi-seed adjoint", *m, f);
      CHECK((!(got & SEL) || ((got & ADJ) && (got & MULTI))) && (!(got & RECORD) || (got & (ADJ | MODEL | LIMIT)) == (ADJ | MODEL | LIMIT)) &&
                (!(got & (MODEL | LIMIT)) || (got & ADJ)) && (!(got & (ADJ | MULTI)) || (got & SOLVE)),
            "move %c from %d: a result without its input", *m, f);
      CHECK(!r.has_prediction() && !r.has_selection() && !r.has_margins() && !r.has_certificate() && !r.has_gains() && !r.has_first_order(),
            "move %c touched another branch", *m);
      if (!seen.count(got)) seen[got] = r, todo.push_back(got);
    }
  }
  // the 18 states of the branch without the chain (tests/src/adjoint_multi_plan_on_host.cpp), and every one of them that has a multi-seed
  // adjoint -- itself, the 5 single-launch chains beside it, the 5 selections -- once more with the chain standing
  CHECK(seen.size() == 18 + 11, "%zu states reached", seen.size());
  printf("%d problems\n", bad);
  return bad != 0;
}
