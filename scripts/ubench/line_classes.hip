// line_classes.hip -- microbenchmark: what a gather of ONE 128-byte line per random row costs, by the ADDRESS of the line.
// The 64-column stream kernel's second column panel (bytes 256..511 of 512-byte rows) runs 12 % slower than its first
// (scripts/exp_panels.py, DESIGN_HISTORY.md section 8): by single lines, the one at byte 384 of every 512.  This program takes the
// kernel away and asks the memory system alone: every wave instruction is a 64-lane dwordx4 gather of 8 rows x 8 lanes x 16 B
// (one full line per row, 1 KiB per instruction), 16 gathers in flight per wave (hand-counted waits, as mode D of
// gather_paths.hip), 8 waves per CU -- the stream kernel's occupancy and depth.
//   table A  "class": the line's address bits [10:7] are fixed to c = 0..15, all higher bits random: address = base + r * 2048 +
//            c * 128.  Which row of which pitch that is follows from the address (pitch 512: row 4r + c / 4, byte (c % 4) * 128;
//            pitch 1024: row 2r + c / 8, byte (c % 8) * 128) -- the two pitches name the SAME set of lines, so the class table is
//            printed once per table size and holds for both.
//   table B  "offset": what a column panel really does -- the byte offset inside the row is fixed, the ROW is random over all
//            rows of the table, at pitch 512 (4 offsets: bits [8:7] fixed, bit 9 up random) and pitch 1024 (8 offsets: bits
//            [9:7] fixed, bit 10 up random).
// Both from a table inside every XCD's L2 (1 MB) and from one of the Reddit shape's operand (232,965 rows x 512 B = 119 MB).
// Prints clocks per 1-KiB gather per CU (and TB/s) per class and table.
// build: hipcc -O3 --offload-arch=gfx950 scripts/ubench/line_classes.hip -o scripts/ubench/line_classes ; run: scripts/ubench/line_classes
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

typedef __attribute__((__vector_size__(4 * sizeof(int)))) int v4i_t;
typedef int v4i_rsrc_t __attribute__((ext_vector_type(4)));

constexpr int DEPTH = 16;        // gathers in flight per wave

// every gather: 8 rows (one per group of 8 lanes), row = a per-group LCG draw in [0, units); byte = row * unit_bytes + off + lane-in-group * 16
__global__ __launch_bounds__(256, 2) void line_kernel(const float *table, unsigned table_bytes, unsigned units, unsigned unit_bytes, unsigned off,
                                                      int steps, float *out) {
   __shared__ float occupancy_pad[16384];                // 64 KB per workgroup: two workgroups (8 waves) per CU, as the stream kernel
   occupancy_pad[threadIdx.x] = 0.0f;
   const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
   const int g = lane >> 3, lc = lane & 7;
   v4i_rsrc_t rs;
   {
      const uint64_t base = (uint64_t)table;
      rs.x = (int)(uint32_t)base; rs.y = (int)(uint32_t)(base >> 32); rs.z = (int)table_bytes; rs.w = 0x00020000;   // range-checked: nothing outside the table is read
   }
   unsigned seed = (blockIdx.x * 4 + wave) * 8 + g + 12345u;
   auto next_off = [&]() -> unsigned {
      seed = seed * 1664525u + 1013904223u;
      return ((seed >> 8) % units) * unit_bytes + off + (unsigned)lc * 16u;
   };
   float acc[4] = {0.f, 0.f, 0.f, 0.f};
   v4i_t tt[DEPTH];
#pragma unroll
   for (int u = 0; u < DEPTH; u++) asm volatile("buffer_load_dwordx4 %0, %1, %2, 0 offen" : "=v"(tt[u]) : "v"(next_off()), "s"(rs));
   for (int s = 0; s < steps; s += DEPTH) {
#pragma unroll
      for (int u = 0; u < DEPTH; u++) {
         asm volatile("s_waitcnt vmcnt(%1)" : "+v"(tt[u]) : "n"(DEPTH - 1));
#pragma unroll
         for (int v = 0; v < 4; v++) acc[v] += __int_as_float(tt[u][v]);
         asm volatile("buffer_load_dwordx4 %0, %1, %2, 0 offen" : "=v"(tt[u]) : "v"(next_off()), "s"(rs));
      }
   }
   asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
   for (int u = 0; u < DEPTH; u++) asm volatile("" : "+v"(tt[u]));
   if (acc[0] + acc[1] + acc[2] + acc[3] + occupancy_pad[(threadIdx.x + 1) & 255] == 123.456f) out[0] = acc[0];
}

static double run(const float *table, size_t table_bytes, unsigned units, unsigned unit_bytes, unsigned off, int steps, float *out, int cus, double mhz,
                  double *tbps) {
   if ((size_t)units * unit_bytes > table_bytes || off + 128 > unit_bytes) { fprintf(stderr, "bad geometry\n"); exit(1); }
   const int blocks = cus * 2;
   hipEvent_t a, b;
   (void)hipEventCreate(&a); (void)hipEventCreate(&b);
   for (int w = 0; w < 2; w++) hipLaunchKernelGGL(line_kernel, dim3(blocks), dim3(256), 0, 0, table, (unsigned)table_bytes, units, unit_bytes, off, steps, out);
   (void)hipEventRecord(a, 0);
   const int reps = 5;
   for (int w = 0; w < reps; w++) hipLaunchKernelGGL(line_kernel, dim3(blocks), dim3(256), 0, 0, table, (unsigned)table_bytes, units, unit_bytes, off, steps, out);
   (void)hipEventRecord(b, 0);
   if (hipEventSynchronize(b) != hipSuccess) { fprintf(stderr, "launch failed: %s\n", hipGetErrorString(hipGetLastError())); exit(1); }
   float ms = 0.f;
   (void)hipEventElapsedTime(&ms, a, b);
   (void)hipEventDestroy(a); (void)hipEventDestroy(b);
   ms /= reps;
   const double gathers = (double)steps * blocks * 4;
   if (tbps) *tbps = gathers * 1024.0 / (ms * 1e-3) / 1e12;
   return ms * 1e-3 * mhz * 1e6 * cus / gathers;           // clocks per 1-KiB gather per CU
}

int main(int argc, char **argv) {
   const int steps = argc > 1 ? atoi(argv[1]) : 8192;
   hipDeviceProp_t p;
   if (hipGetDeviceProperties(&p, 0) != hipSuccess) { fprintf(stderr, "no device\n"); return 1; }
   const int cus = p.multiProcessorCount;
   const double mhz = p.clockRate / 1000.0;
   const size_t sizes[2] = {(size_t)1 << 20, (size_t)232965 * 512};
   const char *names[2] = {"1 MB table (inside every XCD's L2)", "119 MB table (232,965 rows x 512 B)"};
   float *out;
   (void)hipMalloc(&out, 256);
   printf("device: %s, %d CUs, %.0f MHz; %d gathers of 8 lines (1 KiB) per wave, %d in flight, 8 waves per CU\n", p.name, cus, mhz, steps, DEPTH);
   for (int t = 0; t < 2; t++) {
      float *table;
      const size_t bytes = sizes[t] / 2048 * 2048;
      if (hipMalloc(&table, bytes) != hipSuccess) { fprintf(stderr, "hipMalloc failed\n"); return 1; }
      (void)hipMemset(table, 0, bytes);
      for (int w = 0; w < 8; w++) (void)run(table, bytes, (unsigned)(bytes / 2048), 2048, 0, steps, out, cus, mhz, nullptr);    // clocks and caches settle: not printed
      printf("\n== %s, base %% 4096 = %u ==\n", names[t], (unsigned)((uintptr_t)table & 4095));
      printf("A  class = address bits [10:7] of the line (rows of pitch 512 and of pitch 1024 alike); lines touched: %.1f MB\n", bytes / 16 / 1e6);
      printf("   class  bits  pitch 512: row%%4 byte   pitch 1024: row%%2 byte    clk/gather/CU    TB/s\n");
      for (unsigned c = 0; c < 16; c++) {
         double tb;
         const double clk = run(table, bytes, (unsigned)(bytes / 2048), 2048, c * 128, steps, out, cus, mhz, &tb);
         printf("   %5u  %u%u%u%u  %14u %4u  %15u %4u  %15.2f  %6.2f\n", c, (c >> 3) & 1, (c >> 2) & 1, (c >> 1) & 1, c & 1, c / 4, (c % 4) * 128, c / 8,
                (c % 8) * 128, clk, tb);
      }
      for (unsigned pitch = 512; pitch <= 1024; pitch *= 2) {
         printf("B  pitch %u: byte offset of the line inside the row fixed, row random over all %u rows; lines touched: %.1f MB\n", pitch,
                (unsigned)(bytes / pitch), bytes / pitch * 128 / 1e6);
         printf("   offset    clk/gather/CU    TB/s\n");
         for (unsigned o = 0; o < pitch; o += 128) {
            double tb;
            const double clk = run(table, bytes, (unsigned)(bytes / pitch), pitch, o, steps, out, cus, mhz, &tb);
            printf("   %6u  %15.2f  %6.2f\n", o, clk, tb);
         }
      }
      (void)hipFree(table);
   }
   (void)hipFree(out);
   return 0;
}
