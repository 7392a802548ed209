/* TEST INFRASTRUCTURE ONLY.  The eight libecg entry points the reference's EC layer reaches through
 * include/jerasure_shim/, answered on the CPU by this directory's restatement (jerasure_w8.c).  Linked into
 * _ref/ref_ec_cpu in place of libecg.so, so the reference's own classes run where there is no GPU. */
#include <stdint.h>

#include "../include/ecg.h"

int *orc_reed_sol_vandermonde_coding_matrix(int k, int m);
int *orc_cauchy_good_general_coding_matrix(int k, int m);
int orc_invert_matrix(int *mat, int *inv, int rows);
int *orc_matrix_multiply(const int *m1, const int *m2, int r1, int c1, int r2, int c2);
void orc_region_xor(const uint8_t *src, uint8_t *dst, long n);
void orc_matrix_encode(int k, int m, const int *matrix, uint8_t **data, uint8_t **coding, long size);
int orc_matrix_decode(int k, int m, const int *matrix, int row_k_ones, const int *erasures, uint8_t **data,
                      uint8_t **coding, long size);

const char *ecg_last_error(void) { return "cpu backend"; }

int *ecg_reed_sol_vandermonde_coding_matrix(int k, int m, int w)
{
    return w == 8 ? orc_reed_sol_vandermonde_coding_matrix(k, m) : 0;
}

int *ecg_cauchy_good_general_coding_matrix(int k, int m, int w)
{
    return w == 8 ? orc_cauchy_good_general_coding_matrix(k, m) : 0;
}

int ecg_jerasure_invert_matrix(int *mat, int *inv, int rows, int w)
{
    return w == 8 ? orc_invert_matrix(mat, inv, rows) : -1;
}

int *ecg_jerasure_matrix_multiply(int *m1, int *m2, int r1, int c1, int r2, int c2, int w)
{
    return w == 8 ? orc_matrix_multiply(m1, m2, r1, c1, r2, c2) : 0;
}

int ecg_galois_region_xor(char *src, char *dest, int nbytes)
{
    orc_region_xor((const uint8_t *)src, (uint8_t *)dest, nbytes);
    return 0;
}

int ecg_jerasure_matrix_encode(int k, int m, int w, int *matrix, char **data_ptrs, char **coding_ptrs, int size)
{
    if (w != 8) return ECG_EINVAL;
    orc_matrix_encode(k, m, matrix, (uint8_t **)data_ptrs, (uint8_t **)coding_ptrs, size);
    return 0;
}

int ecg_jerasure_matrix_decode(int k, int m, int w, int *matrix, int row_k_ones, int *erasures, char **data_ptrs,
                               char **coding_ptrs, int size)
{
    if (w != 8) return ECG_EINVAL;
    return orc_matrix_decode(k, m, matrix, row_k_ones, erasures, (uint8_t **)data_ptrs, (uint8_t **)coding_ptrs,
                             size);
}
