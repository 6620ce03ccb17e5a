// das_tile_inst.hip -- the instantiations of the tiled kernel for ONE launch configuration (-DQDAS_TILE_CFG=<row of das_tile_cfg.h CFGS>): the Makefile
// compiles this file once per row that has a translation unit, so that they compile in parallel (make -j).  Included by das_tile.hip under -DQDAS_UNITY,
// where the launcher table instantiates every such row in one translation unit.
#include "das_tile_impl.h"

namespace qdas {

template <int BYTES> struct SampleOf;
template <> struct SampleOf<4> { using type = uint32_t; };      // fp16 pairs
template <> struct SampleOf<8> { using type = float2; };
template <> struct SampleOf<16> { using type = double2; };

template <int CI> hipError_t launch_tile_cfg(const TileParams &P, unsigned ntiles, size_t lds, hipStream_t s) {
    using ST = typename SampleOf<CFGS[CI].bytes>::type;
    switch (P.flag & 7) {
        case 0: return launch_tile_i<0, ST, CI>(P, ntiles, lds, s);
        case 1: case 4: return launch_tile_i<1, ST, CI>(P, ntiles, lds, s);
        case 2: return launch_tile_i<2, ST, CI>(P, ntiles, lds, s);
        case 3: return launch_tile_i<3, ST, CI>(P, ntiles, lds, s);
        case 5: return launch_tile_i<5, ST, CI>(P, ntiles, lds, s);
    }
    return hipErrorInvalidValue;
}

#ifdef QDAS_TILE_CFG
static_assert(CFGS[QDAS_TILE_CFG].tu, "das_tile_cfg.h: this configuration has no translation unit");
template hipError_t launch_tile_cfg<QDAS_TILE_CFG>(const TileParams &P, unsigned ntiles, size_t lds, hipStream_t s);
#endif

}  // namespace qdas
