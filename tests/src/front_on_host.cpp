// tests/test_front_on_host.py: csrc/hmpc_front.hip -- front_scalars_kernel and the lane bodies of stages A1 / A2 -- compiled for the CPU against
// tests/src/hip_lane_shim (one thread per lane) and compared bit for bit with what the Python side wrote next to the records: the oracle's x0,
// Acd, Bcd and Fc.  Each entry is rebuilt from the instance's block by the rule the solve kernel's scatter rebuilds it by (front_*_entry of
// hmpc_front.h); the prefix counts are checked against a plain count of the gait bytes.  The program also counts the branches the records
// take; a case marked `wants_branches` must reach every one of them.
//
// File (little endian): int32 n_cases; per case: int32 h, nb, stride, wants_branches; float32 dt, f_max, Ib[3], lt, lh, mu, inv_mass, gravity;
// records [nb][stride] bytes; float32 x0 [nb][13], Acd [nb][169], Bcd [nb][156], Fc [nb][192].
#include <cmath>
#include "hmpc_front.hip"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace hmpc;

static int bad = 0;
static void differ(const char *what, int cs, int i, int t, float got, float want) {
  if (memcmp(&got, &want, 4) != 0) {
    if (++bad <= 20) printf("case %d instance %d %s[%d]: got %.9g want %.9g\n", cs, i, what, t, got, want);
  }
}

enum { B_FMOD, B_CLAMP, B_Q_PP, B_Q_NP, B_Q_PN, B_Q_NN, B_AY_GT_AX, B_AX_EQ_AY, B_ZERO_ZERO, B_NO_STANCE, B_ALL_STANCE, B_COUNT };
static const char *B_NAME[B_COUNT] = {"fmod arm of a joint angle", "pitch at the clamp", "atan2 x>0 y>0", "atan2 x<0 y>0", "atan2 x>0 y<0", "atan2 x<0 y<0",
                                      "atan2 |y| > |x|", "atan2 |x| == |y|", "atan2(0, 0)", "no stance at all", "every leg-step in stance"};

static void count_branches(const float *rf, const unsigned char *gait, int h, float f_max, long *cnt) {
  using RL = RecLayout<2>;
  const double PI = 3.14159265359, PI2 = 2 * PI;
  for (int i = 0; i < 10; ++i) {
    float a = rf[RL::JA + i];
    const int k = i % 5;
    if (k == 2 || k == 4) a = (float)((double)a + 0.3 * PI);
    if (k == 3) a = (float)((double)a - 0.6 * PI);
    if (!(std::fabs((double)a) < PI2)) ++cnt[B_FMOD];
  }
  const float *q = rf + RL::Q;
  if (!(2.0 * (double)(q[0] * q[2] - q[1] * q[3]) < 0.99999)) ++cnt[B_CLAMP];
  for (int which = 0; which < 3; which += 2) {  // roll and yaw: the quadrants of det_atan2
    double y, x;
    if (which == 0) front_euler_args<0>(q, y, x); else front_euler_args<2>(q, y, x);
    if (x > 0 && y > 0) ++cnt[B_Q_PP];
    if (x < 0 && y > 0) ++cnt[B_Q_NP];
    if (x > 0 && y < 0) ++cnt[B_Q_PN];
    if (x < 0 && y < 0) ++cnt[B_Q_NN];
    if (std::fabs(y) > std::fabs(x)) ++cnt[B_AY_GT_AX];
    if (std::fabs(y) == std::fabs(x) && x != 0) ++cnt[B_AX_EQ_AY];
    if (x == 0 && y == 0) ++cnt[B_ZERO_ZERO];
  }
  int st = 0;
  for (int i = 0; i < 2 * h; ++i) st += stance(f_max, gait[i]) ? 1 : 0;
  if (st == 0) ++cnt[B_NO_STANCE];
  if (st == 2 * h) ++cnt[B_ALL_STANCE];
}

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  auto rd = [&](void *p, size_t n) { if (fread(p, 1, n, f) != n) { printf("short file\n"); exit(2); } };
  int n_cases = 0;
  rd(&n_cases, 4);
  long total[B_COUNT] = {};
  for (int cs = 0; cs < n_cases; ++cs) {
    int hd[4];
    float fp[10];
    rd(hd, sizeof(hd)), rd(fp, sizeof(fp));
    const int h = hd[0], nb = hd[1], stride = hd[2], wants = hd[3];
    const float dt = fp[0], f_max = fp[1], mu = fp[7], inv_mass = fp[8], gravity = fp[9];
    std::vector<unsigned char> rec((size_t)nb * stride);
    std::vector<float> x0(nb * 13), Acd(nb * 169), Bcd(nb * 156), Fc(nb * 192);
    rd(rec.data(), rec.size()), rd(x0.data(), 4 * x0.size()), rd(Acd.data(), 4 * Acd.size()), rd(Bcd.data(), 4 * Bcd.size()), rd(Fc.data(), 4 * Fc.size());
    // one block more than the batch, filled with a pattern: the kernel must not write beyond its batch
    std::vector<FrontScalars> blk(nb + 1);
    memset(blk.data(), 0xa5, sizeof(FrontScalars) * blk.size());
    const FrontArgs a = {rec.data(), stride, nb, h, dt, f_max, {fp[2], fp[3], fp[4]}, fp[5], fp[6]};
    if (launch_front_scalars(a, blk.data(), nullptr) != hipSuccess) return 2;
    const unsigned char *tail = reinterpret_cast<const unsigned char *>(&blk[nb]);
    for (size_t t = 0; t < sizeof(FrontScalars); ++t)
      if (tail[t] != 0xa5) { ++bad; printf("case %d: wrote beyond the batch\n", cs); break; }
    long cnt[B_COUNT] = {};
    for (int i = 0; i < nb; ++i) {
      const FrontScalars &F = blk[i];
      const float *rf = reinterpret_cast<const float *>(rec.data() + (size_t)i * stride);
      const unsigned char *gait = reinterpret_cast<const unsigned char *>(rf + RecLayout<2>::NF + 12 * h);
      for (int t = 0; t < 13; ++t) differ("x0", cs, i, t, front_x0_entry(F, rf, t, gravity), x0[i * 13 + t]);
      for (int t = 0; t < 169; ++t) differ("Acd", cs, i, t, front_acd_entry(F, t, dt), Acd[i * 169 + t]);
      for (int t = 0; t < 156; ++t) differ("Bcd", cs, i, t, front_bcd_entry(F, t, dt, inv_mass), Bcd[i * 156 + t]);
      for (int t = 0; t < 192; ++t) differ("Fc", cs, i, t, front_fc_entry(F, t / 12, t % 12, mu), Fc[i * 192 + t]);
      // the prefix counts against a plain count of the gait bytes
      int nl = 0;
      for (int s = 0; s < FRONT_STEPS; ++s) {
        int bits = 0;
        if (s < h) bits = (stance(f_max, gait[2 * s]) ? 1 : 0) | (stance(f_max, gait[2 * s + 1]) ? 2 : 0);
        const int wnl = s < h ? nl : 0, wnv = s < h ? 6 * nl : 0;
        if (F.pre_nl[s] != wnl || F.pre_nv[s] != wnv || F.pre_st[s] != bits) {
          if (++bad <= 20) printf("case %d instance %d step %d: prefix %d %d %d want %d %d %d\n", cs, i, s, F.pre_nl[s], F.pre_nv[s], F.pre_st[s], wnl, wnv, bits);
        }
        nl += (bits & 1) + (bits >> 1);
      }
      if (F.nls != nl || F.n != 6 * nl) { ++bad; printf("case %d instance %d: n %d nls %d want %d %d\n", cs, i, F.n, F.nls, 6 * nl, nl); }
      count_branches(rf, gait, h, f_max, cnt);
    }
    for (int b = 0; b < B_COUNT; ++b) {
      total[b] += cnt[b];
      if (wants && cnt[b] == 0) { ++bad; printf("case %d: no record takes the branch '%s'\n", cs, B_NAME[b]); }
    }
  }
  for (int b = 0; b < B_COUNT; ++b) printf("%-28s %ld\n", B_NAME[b], total[b]);
  printf("%d problems\n", bad);
  return bad != 0;
}
