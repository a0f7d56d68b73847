// The built-in envs' arithmetic, stated ONCE for the host envs (jh_env.hip) and the device-resident envs (jh_devroll.hip): constants,
// the per-env splitmix64 reset stream, one CartPole step, one element of a control step.  float64 throughout; the reset stream is integer
// arithmetic plus `-0.05 + 0.1 u`, so host and device resets agree bit for bit; sin / cos are the caller's library's (the device's may
// differ from the host's in the last bits).
#pragma once
#include <math.h>
#include <stdint.h>

#ifdef __HIPCC__
#define JH_ENV_HD __host__ __device__
#else
#define JH_ENV_HD
#endif

namespace jh_env {
constexpr double kGrav = 9.8, kMc = 1.0, kMp = 0.1, kLen = 0.5, kFmag = 10.0, kTau = 0.02;
constexpr double kThetaLim = 12.0 * 2.0 * 3.14159265358979323846 / 360.0;
constexpr double kXLim = 2.4;
constexpr int64_t kMaxSteps = 500;          // CartPole-v1
constexpr float kRewardStep = 0.1f, kRewardDone = -1.0f;  // gym_env.py:78
constexpr int64_t kControlMaxSteps = 1000;
constexpr double kControlLim = 2.0;
constexpr int kControlMaxS = 64, kControlMaxA = 16;

JH_ENV_HD inline uint64_t seed_word(uint64_t seed, int w) { return seed * 0x9E3779B97F4A7C15ull + (uint64_t)(w + 1) * 0xBF58476D1CE4E5B9ull; }

JH_ENV_HD inline double next_u01(uint64_t& st) {
  st += 0x9E3779B97F4A7C15ull;
  uint64_t x = st;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  x = x ^ (x >> 31);
  return (double)(x >> 11) * (1.0 / 9007199254740992.0);
}

// U(-0.05, 0.05)^S from the env's own stream, step count back to 0 (both envs)
JH_ENV_HD inline void reset_row(double* s, int S, uint64_t& rng, int64_t& t) {
  for (int k = 0; k < S; ++k) s[k] = -0.05 + 0.1 * next_u01(rng);
  t = 0;
}

// one Euler step of the cart-pole ODE on s = (x, x_dot, theta, theta_dot); -> done
JH_ENV_HD inline bool cartpole_advance(double* s, int64_t& t, int64_t action) {
  const double total_mass = kMc + kMp, pml = kMp * kLen;
  double x = s[0], xd = s[1], th = s[2], thd = s[3];
  const double force = action == 1 ? kFmag : -kFmag;
  const double ct = cos(th), st = sin(th);
  const double temp = (force + pml * thd * thd * st) / total_mass;
  const double thacc = (kGrav * st - ct * temp) / (kLen * (4.0 / 3.0 - kMp * ct * ct / total_mass));
  const double xacc = temp - pml * thacc * ct / total_mass;
  x = x + kTau * xd;
  xd = xd + kTau * xacc;
  th = th + kTau * thd;
  thd = thd + kTau * thacc;
  s[0] = x; s[1] = xd; s[2] = th; s[3] = thd;
  t += 1;
  return x < -kXLim || x > kXLim || th < -kThetaLim || th > kThetaLim || t >= kMaxSteps;
}

// the control env's action coupling P[i][j]
inline double control_coupling(int i, int j) { return 0.5 * sin(1.7 * (i + 1) + 2.3 * (j + 1)); }

// s'_i of the control env; `coupling(i, j)` = P[i][j] (the host evaluates it in place, a kernel reads the table the host made from it)
template <class Coupling>
JH_ENV_HD inline double control_next(const double* s, const float* a, int S, int A, int i, Coupling coupling) {
  double drive = 0.0;
  for (int j = 0; j < A; ++j) drive += coupling(i, j) * (double)a[j];
  return 0.95 * s[i] + 0.05 * drive + 0.02 * sin(s[(i + 1) % S]);
}
JH_ENV_HD inline double control_action_cost(const float* a, int A) {
  double a2 = 0.0;
  for (int j = 0; j < A; ++j) a2 += (double)a[j] * (double)a[j];
  return a2;
}
JH_ENV_HD inline bool control_done(double s0, int64_t t) { return s0 > kControlLim || s0 < -kControlLim || t >= kControlMaxSteps; }
JH_ENV_HD inline float control_reward(double s0, double a2) { return (float)(s0 + 0.1 - 0.001 * a2); }
}  // namespace jh_env
