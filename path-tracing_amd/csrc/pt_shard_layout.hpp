// pt_shard_layout.hpp -- the geometry of one rank's tile shard (include/ptx.h, PtxTileShard): the image is cut into tileSize x
// tileSize tiles numbered row-major, and rank r of worldSize owns the tiles t with t % worldSize == r.  Plain host arithmetic with
// no HIP in it: LaunchParams (makeParams), GatherParams, ptx_shard_bytes and the unpack calls are all filled from here.
// The counts are 32-bit, as the kernels' own: numTiles, slotsPerFrame and ownedPixels wrap for absurd extents (a 2^31-1 x 1 image with
// 1024-pixel tiles has 2^21 tiles of 2^20 slots each); ptx_resize and ptx_set_tile_shard refuse nothing on that account.
#pragma once

#include <cstddef>
#include <cstdint>

struct ShardLayout
{
    uint32_t tilesX = 0;        // tiles per row of tiles
    uint32_t numTiles = 0;      // of the whole image
    uint32_t ownedTiles = 0;    // of this rank
    uint32_t slotsPerFrame = 0; // ownedTiles * tileSize^2: the entries of the rank's message, ragged tiles padded
    uint32_t ownedPixels = 0;   // ... of which inside the image
};

inline ShardLayout shardLayout(uint32_t width, uint32_t height, uint32_t rank, uint32_t worldSize, uint32_t tileSize)
{
    ShardLayout s;
    s.tilesX = (width + tileSize - 1) / tileSize;
    const uint32_t tilesY = (height + tileSize - 1) / tileSize;
    s.numTiles = s.tilesX * tilesY;
    s.ownedTiles = s.numTiles > rank ? (s.numTiles - rank + worldSize - 1) / worldSize : 0;
    s.slotsPerFrame = s.ownedTiles * tileSize * tileSize;
    for (uint32_t t = rank; t < s.numTiles; t += worldSize)
    {
        const uint32_t x0 = (t % s.tilesX) * tileSize, y0 = (t / s.tilesX) * tileSize;
        const uint32_t w = width - x0 < tileSize ? width - x0 : tileSize;
        const uint32_t h = height - y0 < tileSize ? height - y0 : tileSize;
        s.ownedPixels += w * h;
    }
    return s;
}
