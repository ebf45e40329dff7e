/* extreme_ray_oracle_check.c — the C oracle's GridHit (oracle/vrt_oracle.c) on the ray and first-hit-camera batches of
 * tests/extreme_queries.py, as a stand-alone program to be built with a sanitizer on the CPU:
 *   clang -std=c11 -g -O1 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all tools/extreme_ray_oracle_check.c oracle/vrt_oracle.c -lm -o extreme_ray_oracle_check
 *   python -m tests.test_extreme_queries export DIR && ./extreme_ray_oracle_check DIR/rays_*.bin
 * The batches hold directions whose squared length overflows or underflows, origins 1e30 from the grid, raw directions of 1e-45 and
 * 3e38 and camera pixels of all of those: this run is what checks the oracle's float -> int conversions (vrt_f2i), its array indices
 * and its loops' ends for undefined behaviour.  A file is what the test exported: the brick dimension, the number of rays, the byte
 * lengths of the seven scene arrays (the grid state, the materials, bindings 3-7), the arrays (each padded to four bytes), the rays
 * (vrt_ray_query: origin, max_t, direction, flags) and the answers the test recorded (vrt_ray_hit).  The queries' screen is restated
 * here; every answer must be the recorded bytes.  Exit status 0: every file agreed. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

typedef struct {
    const void *grid, *materials, *brick_type_bits, *brick_indices, *brick_solid_mask, *brick_type_and_index, *material_indices;
    uint32_t brick_bytes;
    int32_t brick_dimensions;
    float brick_voxel_scale;
} scene_t; /* oracle_scene, field for field */

int oracle_grid_hit_voxel(const void *scene, const void *pc, const float origin[3], const float dir[3], int raw, float out_point[3],
                          float out_normal[3], float *out_t, uint32_t *out_index, int32_t out_voxel[3]);

typedef struct { float origin[3], max_t, direction[3]; uint32_t flags; } query_t;
typedef struct { float point[3], t, normal[3]; uint32_t material; int32_t voxel[3]; uint32_t hit; } hit_t;

static int finite3(const float v[3]) { return isfinite(v[0]) && isfinite(v[1]) && isfinite(v[2]); }

static int check(const char *path) {
    FILE *f = fopen(path, "rb");
    if (!f) return 1;
    uint32_t head[9];
    if (fread(head, 4, 9, f) != 9) return 2;
    const uint32_t b = head[0], n = head[1];
    void *arrays[7];
    for (int k = 0; k < 7; k++) {
        const size_t bytes = ((size_t)head[2 + k] + 3u) & ~(size_t)3u;
        arrays[k] = malloc(head[2 + k] ? head[2 + k] : 1u); /* exactly as long as the array: the sanitizer sees a read beyond it */
        void *padded = malloc(bytes ? bytes : 1u);
        if (fread(padded, 1, bytes, f) != bytes) return 3;
        memcpy(arrays[k], padded, head[2 + k]);
        free(padded);
    }
    query_t *q = malloc((size_t)n * sizeof *q);
    hit_t *want = malloc((size_t)n * sizeof *want);
    if (fread(q, sizeof *q, n, f) != n || fread(want, sizeof *want, n, f) != n || fgetc(f) != EOF) return 4;
    fclose(f);
    const scene_t scene = {arrays[0], arrays[1], arrays[2], arrays[3], arrays[4], arrays[5], arrays[6], b * b * b / 8u, (int32_t)b, 1.0f / (float)b};
    const uint32_t top = ((const uint32_t *)arrays[0])[1] - 1u; /* voxel_dim_y - 1 */
    uint8_t pc[128] = {0};
    size_t hits = 0, screened = 0;
    for (uint32_t i = 0; i < n; i++) {
        hit_t h;
        memset(&h, 0, sizeof h);
        const float *d = q[i].direction;
        if (finite3(q[i].origin) && finite3(d) && !(d[0] == 0.0f && d[1] == 0.0f && d[2] == 0.0f) && q[i].max_t >= 0.0f) {
            const int found = oracle_grid_hit_voxel(&scene, pc, q[i].origin, d, (int)(q[i].flags & 1u), h.point, h.normal, &h.t, &h.material, h.voxel);
            if (found && h.t <= q[i].max_t) {
                h.hit = 1u;
                h.voxel[1] = (int32_t)top - h.voxel[1]; /* y as insert counts it */
                hits++;
            } else {
                memset(&h, 0, sizeof h);
            }
        } else {
            screened++;
        }
        if (memcmp(&h, &want[i], sizeof h) != 0) {
            printf("%s: ray %u is not as recorded\n", path, i);
            return 5;
        }
    }
    printf("%s: b = %u, %u rays: %zu hits, %zu screened, %zu misses, all as recorded\n", path, b, n, hits, screened, (size_t)n - hits - screened);
    for (int k = 0; k < 7; k++) free(arrays[k]);
    free(q);
    free(want);
    return 0;
}

int main(int argc, char **argv) {
    if (argc < 2) {
        printf("usage: extreme_ray_oracle_check rays_<grid>_b<b>.bin ...\n");
        return 2;
    }
    for (int k = 1; k < argc; k++) {
        const int rc = check(argv[k]);
        if (rc) {
            printf("%s: check %d failed\n", argv[k], rc);
            return rc;
        }
    }
    printf("the oracle answers every extreme batch as recorded\n");
    return 0;
}
