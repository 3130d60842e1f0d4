// Stand-alone check of csrc/sph_select.h and csrc/sph_bins.h (tests/test_select_cpu.py builds
// and runs it with a host compiler): every helper hands its lambda the constant it was told to,
// a value outside a list takes the declared fall-back, and nested helpers compose; with
// arguments it prints the bin geometry fill_qbins computes from them.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>

#include "sph_bins.h"
#include "sph_select.h"

static int g_fail = 0;
#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      std::printf("FAILED line %d: %s\n", __LINE__, #c);           \
      g_fail++;                                                    \
    }                                                              \
  } while (0)

// two shape tables in the form of SPH_BLK_SHAPES (three constants) and SPH_ROW2_TILES (two),
// with gaps in their indices
#define TEST_SHAPES3(X) X(0, 64, 8, 4) X(1, 32, 8, 4) X(4, 32, 16, 2)
#define TEST_SHAPES2(X) X(3, 8, 4) X(7, 16, 2)
namespace sph {
SPH_SHAPE_SELECT(select_shape3, TEST_SHAPES3)
SPH_SHAPE_SELECT(select_shape2, TEST_SHAPES2)
}  // namespace sph
using namespace sph;

// the constant a run-time int was turned into by select_int<-1, 1, 3, 2, 8, 17>, and how
// often the lambda ran
static void pick(int v, int *got, int *calls) {
  select_int<-1, 1, 3, 2, 8, 17>(v, [&](auto c) {
    static_assert(std::is_same_v<decltype(c), std::integral_constant<int, decltype(c)::value>>);
    constexpr int C = c;  // (usable as a constant expression: what the launchers rely on)
    *got = std::integral_constant<int, C>::value;
    ++*calls;
  });
}

// `bins dim cutmaxsq lo0 ext0 nb0 lo1 ext1 nb1 lo2 ext2 nb2`: the fields fill_qbins leaves in
// its QBins and Bins, doubles as hexadecimal floats (every bit)
static int print_bins(char **v) {
  double lo[3], ext[3];
  int nb[3];
  for (int k = 0; k < 3; k++) {
    lo[k] = std::strtod(v[2 + 3 * k], nullptr);
    ext[k] = std::strtod(v[3 + 3 * k], nullptr);
    nb[k] = std::atoi(v[4 + 3 * k]);
  }
  QBins q{};
  Bins b{};
  fill_qbins(q, b, lo, ext, nb, std::atoi(v[0]), std::strtod(v[1], nullptr));
  for (int k = 0; k < 3; k++)
    std::printf("axis %d q %a %a %a %d b %a %a %d\n", k, q.lo[k], q.inv[k], q.size[k], q.nb[k],
                b.lo[k], b.inv[k], b.nb[k]);
  std::printf("cutmaxsq %a\n", q.cutmaxsq);
  return 0;
}

int main(int argc, char **argv) {
  static_assert(!STUDY_BUILD, "built without SPH_STUDY");
  if (argc == 13 && std::strcmp(argv[1], "bins") == 0) return print_bins(argv + 2);

  // key_bits: the radix sort's bits cover the keys [0, n), at least one and at most 31
  CHECK(key_bits(1) == 1 && key_bits(2) == 1 && key_bits(3) == 2 && key_bits(4) == 2 &&
        key_bits(5) == 3 && key_bits(1 << 26) == 26 && key_bits((1 << 26) + 1) == 27 &&
        key_bits(0x7fffffff) == 31);

  // select_bool: true and false give their own constants, one call each
  for (int b = 0; b < 2; b++) {
    int calls = 0, got = -1;
    bool is_true_type = false, is_false_type = false;
    select_bool(b != 0, [&](auto c) {
      constexpr bool C = c;
      got = C ? 1 : 0;
      is_true_type = std::is_same_v<decltype(c), std::true_type>;
      is_false_type = std::is_same_v<decltype(c), std::false_type>;
      calls++;
    });
    CHECK(calls == 1 && got == b && is_true_type == (b == 1) && is_false_type == (b == 0));
  }

  // select_int: every listed value gives its own constant, every other the fall-back
  for (int v = -40; v <= 40; v++) {
    const bool listed = v == 1 || v == 3 || v == 2 || v == 8 || v == 17;
    int got = 12345, calls = 0;
    pick(v, &got, &calls);
    CHECK(calls == 1 && got == (listed ? v : -1));
  }
  // a fall-back that is also a value of its own (the lanes per row: 8 unless 4 or 16), and
  // an empty list
  for (int v = 0; v <= 32; v++) {
    int got = -1, calls = 0, got0 = -1;
    select_int<8, 4, 16>(v, [&](auto c) { got = c; calls++; });
    select_int<5>(v, [&](auto c) { got0 = c; });
    CHECK(calls == 1 && got == ((v == 4 || v == 16) ? v : 8) && got0 == 5);
  }

  // shape tables: each listed index gives its constants and true, an unlisted one false
  // without a call
  for (int k = -2; k <= 9; k++) {
    int d3[4] = {0, 0, 0, 0}, d2[3] = {0, 0, 0}, n3 = 0, n2 = 0;
    const bool f3 = select_shape3(k, [&](auto sh) {
      static_assert(sizeof(sh.v) == 3 * sizeof(int));
      constexpr int R = sh.v[0], G = sh.v[1], U = sh.v[2];
      d3[0] = R, d3[1] = G, d3[2] = U;
      n3++;
    });
    const bool f2 = select_shape2(k, [&](auto sh) {
      static_assert(sizeof(sh.v) == 2 * sizeof(int));
      constexpr int G = sh.v[0], U = sh.v[1];
      d2[0] = G, d2[1] = U;
      n2++;
    });
    const int e3[3] = {k == 0 ? 64 : (k == 1 || k == 4) ? 32 : 0,
                       (k == 0 || k == 1) ? 8 : k == 4 ? 16 : 0,
                       (k == 0 || k == 1) ? 4 : k == 4 ? 2 : 0};
    const bool in3 = k == 0 || k == 1 || k == 4, in2 = k == 3 || k == 7;
    CHECK(f3 == in3 && n3 == (in3 ? 1 : 0) && d3[0] == e3[0] && d3[1] == e3[1] && d3[2] == e3[2]);
    CHECK(f2 == in2 && n2 == (in2 ? 1 : 0) && d2[0] == (k == 3 ? 8 : k == 7 ? 16 : 0) &&
          d2[1] == (k == 3 ? 4 : k == 7 ? 2 : 0));
    // the caller's fall-back, as the row passes name theirs
    int g = 0, u = 0;
    auto take = [&](auto sh) { g = sh.v[0], u = sh.v[1]; };
    if (!select_shape2(k, take)) take(Dims<8, 4>{});
    CHECK(g == (k == 7 ? 16 : 8) && u == (k == 7 ? 2 : 4));
  }

  // nested: bool x int x shape, every triple; a combination refused with `if constexpr`
  // (here: U = 2 with the flag set) is mapped to the one that exists
  int triples = 0;
  for (int b = 0; b < 2; b++)
    for (int v = 0; v <= 4; v++)
      for (int k = 0; k <= 5; k++) {
        int got[6] = {-1, -1, -1, -1, -1, -1}, calls = 0;
        const bool found = select_shape3(k, [&](auto sh) {
          constexpr int R = sh.v[0], G = sh.v[1], U = sh.v[2];
          select_bool(b != 0, [&](auto bc) {
            constexpr bool B = bc;
            select_int<0, 1, 2>(v, [&](auto vc) {
              constexpr int V = vc;
              constexpr bool FLAG = B && U == 4;
              if constexpr (B && U != 4) static_assert(!FLAG);
              got[0] = R, got[1] = G, got[2] = U, got[3] = B, got[4] = V, got[5] = FLAG;
              calls++;
            });
          });
        });
        const bool in3 = k == 0 || k == 1 || k == 4;
        CHECK(found == in3 && calls == (in3 ? 1 : 0));
        if (in3) {
          const int R = k == 0 ? 64 : 32, G = k == 4 ? 16 : 8, U = k == 4 ? 2 : 4;
          CHECK(got[0] == R && got[1] == G && got[2] == U && got[3] == b &&
                got[4] == ((v == 1 || v == 2) ? v : 0) && got[5] == (b && U == 4));
          triples++;
        }
      }
  CHECK(triples == 2 * 5 * 3);

  if (g_fail) return 1;
  std::printf("select: all checks passed\n");
  return 0;
}
