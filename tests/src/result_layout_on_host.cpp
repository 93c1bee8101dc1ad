// result_layout_on_host.cpp -- the table of the results derived from a solve (csrc/hmpc_results.h) printed on the CPU: for every (contacts,
// horizon) on the command line one line per array, "contacts horizon family array element-size elements-per-instance", families and arrays
// in the table's order.  tests/test_result_layout_on_host.py compiles this with g++ under AddressSanitizer and UndefinedBehaviorSanitizer
// and compares every line with the shape table interface.py allocates from.  The header is all this includes: no HIP runtime.
#include <stdio.h>
#include <stdlib.h>

#include "hmpc_results.h"

int main(int argc, char **argv) {
  if (argc < 3 || argc % 2 != 1) {
    fprintf(stderr, "usage: %s contacts horizon [contacts horizon ...]\n", argv[0]);
    return 2;
  }
  for (int i = 1; i + 1 < argc; i += 2) {
    const int nc = atoi(argv[i]), hz = atoi(argv[i + 1]);
    for (int f = 0; f < hmpc::N_FAMILIES; ++f) {
      const hmpc::ResultFamily &fam = hmpc::FAMILIES[f];
      for (int k = 0; k < fam.n; ++k)
        printf("%d %d %s %s %zu %zu\n", nc, hz, fam.name, fam.arrays[k].name, fam.arrays[k].elem, fam.arrays[k].row((size_t)nc, (size_t)hz));
    }
  }
  // the chain's rows ARE the record, model and limit rows (the same functions, not equal literals)
  const hmpc::ResultArray *src[hmpc::CHAIN_ARRAYS] = {&hmpc::RECORD_ROWS[0], &hmpc::RECORD_ROWS[1], &hmpc::RECORD_ROWS[2], &hmpc::MODEL_ROWS[3], &hmpc::LIMIT_ROWS[0],
                                                      &hmpc::LIMIT_ROWS[5], &hmpc::MODEL_ROWS[0], &hmpc::MODEL_ROWS[1], &hmpc::MODEL_ROWS[2], &hmpc::MODEL_ROWS[4],
                                                      &hmpc::LIMIT_ROWS[1], &hmpc::LIMIT_ROWS[2], &hmpc::LIMIT_ROWS[3], &hmpc::LIMIT_ROWS[4]};
  int problems = 0;
  for (int k = 0; k < hmpc::CHAIN_ARRAYS; ++k)
    if (hmpc::CHAIN_ROWS[k].row != src[k]->row || hmpc::CHAIN_ROWS[k].elem != src[k]->elem) ++problems, printf("chain row %d is not the row it is taken from\n", k);
  printf("%d problems\n", problems);
  return problems != 0;
}
