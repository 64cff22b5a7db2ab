// The MI x NI accumulator tiles of a GEMM wave, zeroed.  Shared as text by the five tiled GEMM kernels (as a function over the array four
// of them moved).  Expects the constants MI and NI; leaves f32x16 acc[MI][NI].
  f32x16 acc[MI][NI];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NI; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
