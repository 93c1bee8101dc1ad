// csrc/hmpc_record.h on the host, with the system compiler (tests/test_record_layout.py builds this with AddressSanitizer and
// UBSan and runs it as a program).  It includes nothing of the project but that header.
//
//   record_layout_on_host CASES
//
// CASES: binary64 values, case after case: nc, h, f_max, then the fields in the order p v q w r joint_angles yaw weights Alpha_K
// [Rhand f_max_hand] traj gait.  For every case the program prints the layout the header gives for (nc, h), the record packed
// from the binary64 values and from the same values narrowed to binary32 first (hex; each packed into a heap block of exactly
// `stride` bytes) and the record's stance count; then the stance rule over a grid of caps and gait bytes.
#include <stdio.h>
#include <stdlib.h>

#include <type_traits>
#include <vector>

#include "hmpc_record.h"

using namespace hmpc;

static void print_hex(const char *tag, int nc, int h, const unsigned char *rec, int n) {
  printf("pack %d %d %s ", nc, h, tag);
  for (int i = 0; i < n; ++i) printf("%02x", rec[i]);
  printf("\n");
}

template <int NC>
static void one_case(int h, float f_max, const double *x) {
  using RL = RecLayout<NC>;
  static_assert(rec_fixed_floats(NC) == RL::NF, "the run-time view and the template agree");
  const int stride = rec_stride(NC, h);
  const struct { const char *name; int off, len; } fields[] = {
      {"p", RL::P, RL::P_N}, {"v", RL::V, RL::V_N}, {"q", RL::Q, RL::Q_N}, {"w", RL::W, RL::W_N}, {"r", RL::R, RL::R_N},
      {"joint_angles", RL::JA, RL::JA_N}, {"yaw", RL::YAW, RL::YAW_N}, {"weights", RL::WT, RL::WT_N}, {"Alpha_K", RL::AL, RL::AL_N},
      {"Rhand", RL::RH, RL::RH_N}, {"f_max_hand", RL::FMH, RL::FMH_N}, {"traj", RL::NF, 12 * h}};
  for (const auto &f : fields)
    if (f.len) printf("field %d %d %s %d %d\n", NC, h, f.name, f.off, f.len);
  printf("sizes %d %d fixed=%d gait_offset=%d payload=%d stride=%d\n", NC, h, rec_fixed_floats(NC), rec_gait_offset(NC, h),
         rec_payload_bytes(NC, h), stride);

  // the sources, in the order of CASES
  const int nfix = RL::NF, nval = nfix + 12 * h + NC * h;
  std::vector<double> d(x, x + nval);
  std::vector<float> s(nval);
  for (int i = 0; i < nval; ++i) s[i] = (float)d[i];
  std::vector<int> gi(NC * h);
  std::vector<unsigned char> gb(NC * h);
  for (int i = 0; i < NC * h; ++i) gi[i] = (int)d[nfix + 12 * h + i], gb[i] = (unsigned char)gi[i];
  auto source = [&](auto *v, auto *g) {
    using T = std::remove_const_t<std::remove_pointer_t<decltype(v)>>;
    using G = std::remove_const_t<std::remove_pointer_t<decltype(g)>>;
    RecSource<T, G> r{v + RL::P, v + RL::V, v + RL::Q, v + RL::W, v + RL::R, v + RL::JA, v[RL::YAW], v + RL::WT, v + RL::NF, v + RL::AL, g};
    if (NC == 3) r.Rhand = v + RL::RH, r.f_max_hand = v[RL::FMH];
    return r;
  };
  unsigned char *rec = (unsigned char *)malloc(stride);  // exactly the stride: a write past the record ends the run
  pack_record<NC>(rec, h, source(d.data(), gi.data()));
  print_hex("double", NC, h, rec, stride);
  printf("count %d %d %d\n", NC, h, rec_stance_count(rec, NC, h, f_max));
  free(rec);
  rec = (unsigned char *)malloc(stride);
  pack_record<NC>(rec, h, source(s.data(), gb.data()));
  print_hex("float", NC, h, rec, stride);
  free(rec);
}

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  FILE *fp = fopen(argv[1], "rb");
  if (!fp) return 2;
  std::vector<double> x;
  double buf[256];
  for (size_t n; (n = fread(buf, sizeof(double), 256, fp)) > 0;) x.insert(x.end(), buf, buf + n);
  fclose(fp);
  for (size_t at = 0; at < x.size();) {
    if (at + 3 > x.size()) return 3;
    const int nc = (int)x[at], h = (int)x[at + 1];
    const float f_max = (float)x[at + 2];
    if ((nc != 2 && nc != 3) || h < 1 || h > 20) return 3;
    const size_t nval = (size_t)rec_fixed_floats(nc) + 12 * h + nc * h;
    if (at + 3 + nval > x.size()) return 3;
    if (nc == 2) one_case<2>(h, f_max, &x[at + 3]);
    else one_case<3>(h, f_max, &x[at + 3]);
    at += 3 + nval;
  }
  const float caps[] = {0.f, 5e-5f, 9.99e-5f, 1e-4f, -1.f, 500.f};
  for (float cap : caps)
    for (int g = 0; g < 3; ++g) printf("stance %a %d %d\n", (double)cap, g, stance(cap, (unsigned char)g) ? 1 : 0);
  printf("done\n");
  return 0;
}
