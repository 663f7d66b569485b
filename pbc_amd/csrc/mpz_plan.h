// mpz_plan.h -- the digit string of element_mul_mpz / element_pow_mpz (include/pbc_hip.h pbc_hip_element_mul_mpz_batch):
// ONE non-negative integer k for a whole batch, given as a big-endian magnitude of any length up to kMpzMaxBytes, recoded
// once on the host into the signed digits every lane of the kernels (group_mpz.cuh) walks.  Pure host code, no HIP: the
// library, the host mirror of the tests and pbc_hip_diag_mpz_digits share it.
//
// w >= 2: width-w NAF.  Digit i (weight 2^i) is zero or odd with |d| < 2^(w-1); a non-zero digit is followed by at least
// w - 1 zeros; the top digit is positive; at most bits(k) + 1 <= 8 klen + 1 digits.  w = 2 is the plain NAF (digits -1, 0,
// +1).  w = 1: the bits of k (the GT kernels: there is no cheap inverse in a field, so no negative digits).
// k = 0 (no bytes, or zero bytes only) gives the empty string.  The string has no end marker: its LENGTH travels to the
// kernels as a kernel argument.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace pbc_host {

constexpr size_t kMpzMaxBytes = 512;   // PBC_HIP_MPZ_MAX_BYTES
constexpr int kMpzMaxWidth = 6;        // digits fit an int8_t with room to spare

// bit i of the big-endian magnitude k (zero beyond its bytes)
inline unsigned mpz_bit(const uint8_t *k, size_t klen, size_t i) {
  return (i >> 3) < klen ? (k[klen - 1 - (i >> 3)] >> (i & 7)) & 1u : 0u;
}
// bit length of k: 0 for k = 0 (leading zero bytes do not count)
inline size_t mpz_bits(const uint8_t *k, size_t klen) {
  size_t lead = 0;
  while (lead < klen && k[lead] == 0) lead++;
  if (lead == klen) return 0;
  size_t bits = 8 * (klen - lead);
  for (uint8_t top = k[lead]; !(top & 0x80); top = (uint8_t) (top << 1)) bits--;
  return bits;
}
// out: digit i at index i, the top digit last (non-zero).  Walks the bits once with a carry: at an odd position value
// v = (bits i .. i + w - 1) + carry mod 2^w the digit is v, or v - 2^w from the upper half; what is left of the window is
// 0 or 2^w, the next carry.
inline void mpz_digits(const uint8_t *k, size_t klen, int w, std::vector<int8_t> &out) {
  out.clear();
  const size_t nb = mpz_bits(k, klen);
  if (w < 1) w = 1;
  if (w > kMpzMaxWidth) w = kMpzMaxWidth;
  if (w == 1) {
    for (size_t i = 0; i < nb; i++) out.push_back((int8_t) mpz_bit(k, klen, i));
    return;
  }
  unsigned carry = 0;
  size_t i = 0;
  while (i < nb || carry) {
    if ((mpz_bit(k, klen, i) ^ carry) == 0) {      // even: the carry (bit and carry both 0, or both 1) goes on as it is
      out.push_back(0);
      i++;
      continue;
    }
    unsigned v = carry;
    for (int j = 0; j < w; j++) v += mpz_bit(k, klen, i + (size_t) j) << j;
    const unsigned low = v & ((1u << w) - 1);
    const int d = low >= (1u << (w - 1)) ? (int) low - (1 << w) : (int) low;
    carry = (unsigned) (((int) v - d) >> w);
    out.push_back((int8_t) d);
    for (int j = 1; j < w; j++) out.push_back(0);
    i += (size_t) w;
  }
  while (!out.empty() && out.back() == 0) out.pop_back();
}

// The digits of ONE call and their width.  GT: the bits of k (w = 1).  Points: the plain NAF (w = 2: the kernels add +-P,
// no table) or the width-4 NAF (a per-lane table of P, 3P, 5P, 7P), whichever does less work for THIS k -- the table costs
// three additions, a doubling, an inversion and the normalisation of its entries, about ten additions' worth, so it is
// taken when it saves more than that: long dense integers (a random k of Z_r length: about 53 against 32 additions), not
// an r of Solinas form, a power of two or 2^64 + 1.
constexpr long kMpzTableGain = 10;
inline int mpz_recode(bool gt, const uint8_t *k, size_t klen, std::vector<int8_t> &digits) {
  if (gt) { mpz_digits(k, klen, 1, digits); return 1; }
  std::vector<int8_t> wide;
  mpz_digits(k, klen, 2, digits);
  mpz_digits(k, klen, 4, wide);
  long nz2 = 0, nz4 = 0;
  for (int8_t d : digits) nz2 += d != 0;
  for (int8_t d : wide) nz4 += d != 0;
  if (nz2 - nz4 <= kMpzTableGain) return 2;
  digits.swap(wide);
  return 4;
}

// GT of type f on the five-word fields: element_pow_zn's cyclotomic lane (group_ops.cuh f_gt_pow_cyc_lane: Granger-Scott
// squarings, signed 4-bit windows, behind its own per-lane membership test) takes k as a Z_r RECORD and does the same work
// whatever k is; the generic square-and-multiply of this call pays a full F_q^12 squaring per bit and a product per set
// bit.  Measured on f.param (profiles/mul_mpz_notes.md): the cyclotomic lane costs what ~0.67 generic squarings per bit
// of the RECORD cost, a generic product ~1.5 generic squarings -- so a k that fits the record goes to the cyclotomic
// lane when 2 bits + 3 set bits exceeds 1.4 x 8 zlen (dense exponents: 2.2x faster there) and stays on the generic lane
// otherwise (2^64 + 1: 1.5x faster here).
inline bool mpz_gt_wants_record(const std::vector<int8_t> &bits, size_t zlen) {
  long set = 0;
  for (int8_t b : bits) set += b != 0;
  return bits.size() <= 8 * zlen && 10 * (2 * (long) bits.size() + 3 * set) > 14 * 8 * (long) zlen;
}

}  // namespace pbc_host
