// pt_scene_host.hpp -- host side of the scene: ptx_share_scene, ptx_scene_upload and the streamed textures.  An upload is a checked plan, then named
// stages: validateSceneDesc, flattenScene and planTextures read the description only and hold every PTX_ERROR_INVALID_ARGUMENT
// refusal, so a refused description leaves the handle as it was; uploadGeometry, uploadTextures and alphaFootprints then write
// r->scene in place.  Included by pt_runtime.hpp below the renderer object (PtxRenderer, SceneData, DevBuf, HIP_TRY, fail) and
// ahead of pt_bvh_host.hpp; a stage returns a PTX_* code, and the host-only ones take the handle for fail() alone.
#pragma once

// Does the material's branch of material.glsl:62-142 fetch a scene texture (an index at or past PTX_SCENE_TEXTURE_OFFSET inside
// the uploaded table) through any of its five slots?  The five indices sit at the same offsets in the three 96-byte structs.
static bool materialSamplesSceneTexture(const PtxSceneDesc *s, uint32_t materialId)
{
    const uint32_t type = materialId & 0xffu, index = materialId >> 8;
    const uint32_t *idx = nullptr;
    if (type == PTX_MATERIAL_TYPE_METALLIC_ROUGHNESS && index < s->metallicRoughnessMaterialCount)
        idx = &s->metallicRoughnessMaterials[index].EmissiveIdx;
    else if (type == PTX_MATERIAL_TYPE_SPECULAR_GLOSSINESS && index < s->specularGlossinessMaterialCount)
        idx = &s->specularGlossinessMaterials[index].EmissiveIdx;
    else if (type == PTX_MATERIAL_TYPE_PHONG && index < s->phongMaterialCount)
        idx = &s->phongMaterials[index].EmissiveIdx;
    if (!idx)
        return false;
    for (int k = 0; k < 5; k++)
        if (idx[k] >= PTX_SCENE_TEXTURE_OFFSET && idx[k] - PTX_SCENE_TEXTURE_OFFSET < s->textureCount)
            return true;
    return false;
}

// world = A_instance * A_mesh * x (sampling.glsl:7)
static void composeTransform(const float *Ai, const float *Am, float *M)
{
    for (int r = 0; r < 3; r++)
    {
        for (int c = 0; c < 3; c++)
            M[r * 4 + c] = (Ai[r * 4 + 0] * Am[0 * 4 + c] + Ai[r * 4 + 1] * Am[1 * 4 + c]) + Ai[r * 4 + 2] * Am[2 * 4 + c];
        M[r * 4 + 3] = ((Ai[r * 4 + 0] * Am[0 * 4 + 3] + Ai[r * 4 + 1] * Am[1 * 4 + 3]) + Ai[r * 4 + 2] * Am[2 * 4 + 3]) + Ai[r * 4 + 3];
    }
}

// inverse of the 3x3 linear part by cofactors * (1/det), columns out
static void inverseLinear(const float *M, float *Rinv)
{
    const float m00 = M[0], m01 = M[4], m02 = M[8]; // column 0 of the math matrix
    const float m10 = M[1], m11 = M[5], m12 = M[9];
    const float m20 = M[2], m21 = M[6], m22 = M[10];
    const float det = (m00 * (m11 * m22 - m21 * m12) - m10 * (m01 * m22 - m21 * m02)) + m20 * (m01 * m12 - m11 * m02);
    const float id = 1.0f / det;
    Rinv[0] = (m11 * m22 - m21 * m12) * id;
    Rinv[3] = -(m10 * m22 - m20 * m12) * id;
    Rinv[6] = (m10 * m21 - m20 * m11) * id;
    Rinv[1] = -(m01 * m22 - m21 * m02) * id;
    Rinv[4] = (m00 * m22 - m20 * m02) * id;
    Rinv[7] = -(m00 * m21 - m20 * m01) * id;
    Rinv[2] = (m01 * m12 - m11 * m02) * id;
    Rinv[5] = -(m00 * m12 - m10 * m02) * id;
    Rinv[8] = (m00 * m11 - m10 * m01) * id;
}

template <typename T> static int upload(PtxRenderer *r, DevBuf<T> &buf, const T *src, size_t count)
{
    HIP_TRY(r, buf.alloc(count));
    if (count)
        HIP_TRY(r, hipMemcpyAsync(buf.p, src, count * sizeof(T), hipMemcpyHostToDevice, r->stream));
    return PTX_OK;
}

static int shareScene(PtxRenderer *r, PtxRenderer *owner)
{
    if (!r || !owner || r == owner)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "ptx_share_scene: need two different renderers");
    if (owner->link.owner || !r->link.sharers.empty())
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "ptx_share_scene: the owner must hold its own scene, and a renderer others share from cannot borrow");
    if (owner->device != r->device)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "ptx_share_scene: renderers on different devices (%d, %d)", r->device, owner->device);
    if (!owner->link.ready || !owner->accel.ready)
        return fail(r, PTX_ERROR_NOT_READY, "ptx_share_scene: the owner needs ptx_scene_upload and ptx_build_accel first");
    HIP_TRY(r, hipSetDevice(r->device));
    // the owner's uploads and build are enqueued on ITS stream: finished before any stream of the borrower reads them;
    // the borrower's own frames in flight end before its scene goes away
    HIP_TRY(r, hipStreamSynchronize(owner->stream));
    HIP_TRY(r, hipStreamSynchronize(r->stream));
    if (r->streams.aux)
        HIP_TRY(r, hipStreamSynchronize(r->streams.aux.get()));
    detachSharedScene(r);
    // its own copies are not needed any more (uploads still streaming into them end first)
    r->scene.streaming.reset();
    r->scene = SceneData();
    r->accel.tree = AccelState::Tree();
    r->accel.build = BuildState();
    r->link.ready = false;
    r->link.owner = owner;
    owner->link.sharers.push_back(r);
    r->accel.ready = true;
    r->launch.hint.forget(); // whatever this handle had learnt, it had learnt on another scene
    r->chain.status.sceneChanged(); // ... and its guides and history lead back to no pose of this one
    r->stats.triangles = owner->stats.triangles;
    r->stats.bvhNodes = owner->stats.bvhNodes;
    r->stats.treeTriangles = owner->stats.treeTriangles;
    r->stats.treeReferences = owner->stats.treeReferences;
    return PTX_OK;
}

// Stage 1: the indices the kernels will dereference (the reference trusts its importer).
static int validateSceneDesc(PtxRenderer *r, const PtxSceneDesc *s)
{
    for (uint32_t i = 0; i < s->instanceCount; i++)
        if (s->instances[i].ModelIndex >= s->modelCount)
            return fail(r, PTX_ERROR_INVALID_ARGUMENT, "instance %u: model index out of range", i);
    for (uint32_t m = 0; m < s->modelCount; m++)
        if ((uint64_t)s->models[m].MeshOffset + s->models[m].MeshCount > s->meshCount)
            return fail(r, PTX_ERROR_INVALID_ARGUMENT, "model %u: mesh range out of bounds", m);
    for (uint32_t k = 0; k < s->meshCount; k++)
    {
        const PtxMeshRecord &rec = s->meshes[k];
        if (rec.GeometryIndex >= s->geometryCount || rec.TransformIndex >= s->transformCount)
            return fail(r, PTX_ERROR_INVALID_ARGUMENT, "mesh %u: geometry/transform index out of range", k);
        const uint32_t type = rec.MaterialId & 0xffu, index = rec.MaterialId >> 8;
        const uint32_t limit = type == PTX_MATERIAL_TYPE_METALLIC_ROUGHNESS    ? s->metallicRoughnessMaterialCount
                               : type == PTX_MATERIAL_TYPE_SPECULAR_GLOSSINESS ? s->specularGlossinessMaterialCount
                               : type == PTX_MATERIAL_TYPE_PHONG               ? s->phongMaterialCount
                                                                               : 0xffffffffu;
        if (type <= PTX_MATERIAL_TYPE_PHONG && index >= limit)
            return fail(r, PTX_ERROR_INVALID_ARGUMENT, "mesh %u: material index out of range", k);
    }
    for (uint32_t g = 0; g < s->geometryCount; g++)
    {
        const PtxGeometry &geo = s->geometries[g];
        // an animated geometry addresses the animated vertex / index arrays (Renderer.cpp:280-312)
        const uint64_t vLimit = geo.IsAnimated ? (s->animatedVertices ? s->animatedVertexCount : 0) : s->vertexCount;
        const uint64_t iLimit = geo.IsAnimated ? (s->animatedIndices ? s->animatedIndexCount : 0) : s->indexCount;
        const uint32_t *idx = geo.IsAnimated ? s->animatedIndices : s->indices;
        if ((uint64_t)geo.VertexOffset + geo.VertexLength > vLimit || (uint64_t)geo.IndexOffset + geo.IndexLength > iLimit)
            return fail(r, PTX_ERROR_INVALID_ARGUMENT, "geometry %u: vertex/index range out of bounds", g);
        for (uint32_t k = 0; k < geo.IndexLength; k++)
            if (idx[geo.IndexOffset + k] >= geo.VertexLength)
                return fail(r, PTX_ERROR_INVALID_ARGUMENT, "geometry %u: index %u beyond its vertex range", g, k);
    }
    return PTX_OK;
}

// Stage 2: (instance, mesh) pairs in instance-then-mesh order; global triangle id = running prim count.
// Device vertex buffer = scene vertices, then one skinned copy per instanced animated mesh in pair order
// (OutAnimatedVertexBuffer, Renderer.cpp:296-303); device index buffer = scene indices, then the animated indices.
struct FlatScene
{
    std::vector<DevPair> pairs;
    std::vector<uint32_t> pairFirst, pairInstance;
    std::vector<DebugPair> debugPairs; // the ids and the winding the debug view shows per pair (pt_debug_view.hpp)
    std::vector<uint32_t> skinSource; // output vertex -> animated vertex (AnimatedVertexMapBuffer)
    std::vector<PtxTransform> pairMeshTransform;
    uint64_t triangles = 0;
    bool anyNonOpaque = false, mixedMaterialTypes = false, mixedTextured = false;
    std::vector<PtxVertex> verts; // staging of uploadGeometry, alive until sceneUpload's last stream synchronisation
    std::vector<uint32_t> inds;
};

static int flattenScene(PtxRenderer *r, const PtxSceneDesc *s, FlatScene &flat)
{
    uint32_t typesSeen = 0; // bit per material type, unknown types share bit 3
    bool textured = false, plain = false;
    for (uint32_t i = 0; i < s->instanceCount; i++)
    {
        const PtxModelInstance &inst = s->instances[i];
        const PtxModel &model = s->models[inst.ModelIndex];
        for (uint32_t k = 0; k < model.MeshCount; k++)
        {
            const PtxMeshRecord &rec = s->meshes[model.MeshOffset + k];
            const PtxGeometry &geo = s->geometries[rec.GeometryIndex];
            DevPair pr;
            composeTransform(inst.Transform.m, s->transforms[rec.TransformIndex].m, pr.M);
            inverseLinear(pr.M, pr.Rinv);
            pr.vertexOffset = geo.VertexOffset;
            pr.indexOffset = geo.IndexOffset;
            if (geo.IsAnimated)
            {
                if (s->vertexCount + flat.skinSource.size() + geo.VertexLength > 0xffffffffull || s->indexCount + s->animatedIndexCount > 0xffffffffull)
                    return fail(r, PTX_ERROR_INVALID_ARGUMENT, "animated meshes exceed the 32-bit vertex / index space");
                pr.vertexOffset = static_cast<uint32_t>(s->vertexCount + flat.skinSource.size());
                pr.indexOffset = static_cast<uint32_t>(s->indexCount + geo.IndexOffset);
                for (uint32_t v = 0; v < geo.VertexLength; v++)
                    flat.skinSource.push_back(geo.VertexOffset + v);
            }
            flat.pairInstance.push_back(i);
            // gl_InstanceID / gl_GeometryIndexEXT of the pair, and whether the instance mirrors: the TLAS instance carries
            // inst.Transform alone (AccelerationStructure.cpp:271), the mesh transform is baked into the BLAS
            flat.debugPairs.push_back(DebugPair{ i, k, transformMirrors(inst.Transform.m) ? kDebugPairMirrored : 0u });
            flat.pairMeshTransform.push_back(s->transforms[rec.TransformIndex]);
            pr.materialId = rec.MaterialId;
            pr.flags = (geo.IsOpaque ? 0u : kPairNonOpaque) | (materialSamplesSceneTexture(s, rec.MaterialId) ? kPairTextured : 0u);
            if (pr.flags & kPairNonOpaque)
                flat.anyNonOpaque = true;
            typesSeen |= 1u << ((pr.materialId & 0xffu) <= PTX_MATERIAL_TYPE_PHONG ? (pr.materialId & 0xffu) : 3u);
            ((pr.flags & kPairTextured) ? textured : plain) = true;
            flat.pairs.push_back(pr);
            flat.pairFirst.push_back(static_cast<uint32_t>(flat.triangles));
            flat.triangles += geo.IndexLength / 3;
        }
    }
    if (flat.triangles > kMaxTriangles)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "scene has %llu triangles; limit is 2^29-1", (unsigned long long)flat.triangles);
    flat.pairFirst.push_back(static_cast<uint32_t>(flat.triangles));
    flat.mixedMaterialTypes = (typesSeen & (typesSeen - 1u)) != 0u;
    flat.mixedTextured = textured && plain;
    return PTX_OK;
}

// per texture: how its level 0 is produced (what lands in the table is its DevTexture)
struct Placement
{
    uint32_t srcW, srcH;  // the file's level 0
    uint32_t fileLevels;  // levels in the caller's data
    uint32_t firstFile;   // file level that becomes level 0 when the file's own chain is used
    bool useFileChain;    // every level comes from the file (TextureUploader.cpp:440,492-501)
    uint32_t halvings;    // blits from the file's level 0 down towards the budgeted extent (:479-490)
    int temp;             // table entry of the scratch chain, or -1
    bool rejected = false; // a block-compressed file the upload rules cannot take: planned as the 1 x 1 white texel
    size_t bcOffset = 0;   // block-compressed: first byte of the kept levels in the block pool (a multiple of 16)
};

struct TexturePlan
{
    uint32_t textureCount = 0, skyKind = PTX_SKYBOX_CLEAR_COLOR;
    uint32_t total = 0; // scene textures, then the skybox images, one level each (TextureUploader.cpp:203-262)
    std::vector<Placement> place;        // [total]
    std::vector<DevTexture> table;       // [total], then the scratch chains: offsets into the pool of the format
    std::vector<DevTexture> renderTable; // [total]: offsets into the decoded pool, the RGBA32F textures first
    size_t n8 = 0, nf = 0;               // texels of the two format pools ...
    size_t scratch8 = 0, scratchF = 0;   // ... and of the scratch region behind each, used by one scaled texture after the other
    size_t nbc = 0, bcBytes = 0;         // block-compressed textures: their decoded texels (behind nf + n8 in the decoded pool), their blocks
    std::vector<uint32_t> rejected;      // scene textures planned as the white texel (ptx_textures_rejected)
    bool samplerNeeded = false;
    std::vector<AlphaTex> alphaTex; // any-hit data: the alpha footprints of every texture some material names as its colour texture
    std::vector<uint32_t> alphaTexOf;
    size_t alphaQuads = 0;
};

static const PtxTextureDesc &textureDescOf(const PtxSceneDesc *s, uint32_t n, uint32_t i) { return i < n ? s->textures[i] : s->skybox[i - n]; }
static uint32_t fullLevels(uint32_t w, uint32_t h)
{
    uint32_t m = w > h ? w : h, levels = 1;
    while (m > 1) { m >>= 1; levels++; } // floor(log2(max)) + 1, Image.cpp:14-17
    return levels > 16u ? 16u : levels;
}
static uint32_t mipDim(uint32_t v, uint32_t l) { return v >> l ? v >> l : 1u; }
// texels of the first `levels` levels of a w x h image
static size_t chainTexels(uint32_t w, uint32_t h, uint32_t levels)
{
    size_t n = 0;
    for (uint32_t l = 0; l < levels; l++)
        n += (size_t)mipDim(w, l) * mipDim(h, l);
    return n;
}
// puts the levels of `t` into its pool from texel `first` on; returns the texel behind them
static size_t placeLevels(DevTexture &t, size_t first)
{
    for (uint32_t l = 0; l < t.levels; l++)
        t.levelOffset[l] = (uint32_t)(first + chainTexels(t.width, t.height, l));
    return first + chainTexels(t.width, t.height, t.levels);
}

// ---- block-compressed formats (pt_bc.hpp; the layout is the text of include/ptx.h) ----
constexpr uint32_t kTextureFormats = PTX_TEXTURE_BC5_UNORM + 1u;
static const uint32_t kWhiteTexel8 = 0xffffffffu; // what a rejected texture holds
static bool isBcFormat(uint32_t f) { return f >= PTX_TEXTURE_BC1_UNORM && f <= PTX_TEXTURE_BC5_UNORM; }
static uint32_t bcBlockBytes(uint32_t f) { return f == PTX_TEXTURE_BC1_UNORM || f == PTX_TEXTURE_BC1_SRGB ? 8u : 16u; }
// bytes of the levels [first, first + levels) of a w x h image: ceil(w_l / 4) * ceil(h_l / 4) blocks each
static size_t bcChainBytes(uint32_t w, uint32_t h, uint32_t first, uint32_t levels, uint32_t format)
{
    size_t blocks = 0;
    for (uint32_t l = first; l < first + levels; l++)
        blocks += (size_t)((mipDim(w, l) + 3u) / 4u) * ((mipDim(h, l) + 3u) / 4u);
    return blocks * bcBlockBytes(format);
}
// the texel data a texture is uploaded from: the caller's, or the white texel of a rejected one
static const void *textureData(const PtxTextureDesc &d, const Placement &pl) { return pl.rejected ? &kWhiteTexel8 : d.data; }

// TextureUploader::DetermineMaxTextureSizes (TextureUploader.cpp:551-569): the largest square extent whose full chain
// fits the per-texture share of the budget (Config.h:63-64,162-163: min(80 % of the device memory, 1 GiB)), per format;
// forceFullTextureSize keeps MaxTextureDataSize = 4096 (TextureUploader.h:74).  A block-compressed format is priced in
// block bytes with the 4 x 4 rounding of every level.
static void maxTextureExtents(const PtxSceneDesc *s, uint32_t textureCount, uint64_t deviceTotalBytes, uint32_t maxExtent[kTextureFormats])
{
    for (uint32_t f = 0; f < kTextureFormats; f++)
        maxExtent[f] = 4096u;
    if (s->forceFullTextureSize || !textureCount || s->textureMemoryBudget == ~0ull)
        return;
    const uint64_t budget = s->textureMemoryBudget ? s->textureMemoryBudget : std::min<uint64_t>(deviceTotalBytes / 100u * 80u, 1024ull << 20);
    for (uint32_t f = 0; f <= PTX_TEXTURE_RGBA32F; f++)
        for (uint32_t &m = maxExtent[f]; m > 1u && chainTexels(m, m, fullLevels(m, m)) * (f == PTX_TEXTURE_RGBA32F ? 16u : 4u) > budget / textureCount;)
            m >>= 1;
    for (uint32_t f = PTX_TEXTURE_BC1_UNORM; f < kTextureFormats; f++)
        for (uint32_t &m = maxExtent[f]; m > 1u && bcChainBytes(m, m, 0, fullLevels(m, m), f) > budget / textureCount;)
            m >>= 1;
}

// The same for a block-compressed file, whose levels can be neither generated nor rescaled (TextureUploader.cpp:401-503 for a
// format outside ScalingFormats): the file's chain, a one-level image, the file's levels from the budgeted extent on, or rejected.
static int placeBcTexture(PtxRenderer *r, uint32_t i, uint32_t mx, DevTexture &t, Placement &pl)
{
    const uint32_t scale = std::max((pl.srcW + mx - 1) / mx, (pl.srcH + mx - 1) / mx);
    const uint32_t full = fullLevels(pl.srcW, pl.srcH);
    if (pl.fileLevels > full)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "texture %u: %u levels for a %u x %u image", i, pl.fileLevels, pl.srcW, pl.srcH);
    t.width = std::max(pl.srcW / scale, 1u);
    t.height = std::max(pl.srcH / scale, 1u);
    pl.useFileChain = true;
    if (scale == 1)
    {
        t.levels = pl.fileLevels == full ? full : 1u; // :423-437: a single-level file stays a single-level image
        pl.rejected = pl.fileLevels != full && pl.fileLevels > 1u; // :444-453
    }
    else
    {
        // :462-476, :492-501; a level `skip` of another extent is rejected here, where the reference would copy mismatching data
        t.levels = fullLevels(t.width, t.height);
        pl.rejected = pl.fileLevels <= 1u || pl.fileLevels < t.levels;
        if (!pl.rejected)
        {
            pl.firstFile = pl.fileLevels - t.levels;
            pl.rejected = mipDim(pl.srcW, pl.firstFile) != t.width || mipDim(pl.srcH, pl.firstFile) != t.height;
        }
    }
    if (pl.rejected)
    {
        pl = { 1u, 1u, 1u, 0u, false, 0u, -1, true };
        t = { 1u, 1u, 1u, PTX_TEXTURE_RGBA8_UNORM, {} };
    }
    return PTX_OK;
}

// One scene texture of at most `mx` texels across (TextureUploader::UploadTexture): its extent and levels into `t`, the way
// its level 0 is produced into `pl`.  A texture that is scaled through a scratch chain gets table entry `nextTemp`.
static int placeSceneTexture(PtxRenderer *r, uint32_t i, uint32_t mx, uint32_t nextTemp, DevTexture &t, Placement &pl, TexturePlan &plan)
{
    // :409-415: integer scale that brings both sides under the limit
    const uint32_t scale = std::max((pl.srcW + mx - 1) / mx, (pl.srcH + mx - 1) / mx);
    t.width = std::max(pl.srcW / scale, 1u);
    t.height = std::max(pl.srcH / scale, 1u);
    t.levels = fullLevels(t.width, t.height);
    if (pl.fileLevels > fullLevels(pl.srcW, pl.srcH))
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "texture %u: %u levels for a %u x %u image", i, pl.fileLevels, pl.srcW, pl.srcH);
    // a file with its own chain: the levels from the budgeted extent down are taken as they are (:492-501)
    const uint32_t skip = pl.fileLevels > t.levels ? pl.fileLevels - t.levels : 0u;
    if (scale == 1)
        pl.useFileChain = pl.fileLevels == t.levels && t.levels > 1;
    else if (skip && mipDim(pl.srcW, skip) == t.width && mipDim(pl.srcH, skip) == t.height)
    {
        pl.useFileChain = true;
        pl.firstFile = skip;
    }
    else
    {
        while (mipDim(pl.srcW, pl.halvings + 1) >= t.width && mipDim(pl.srcH, pl.halvings + 1) >= t.height &&
               (mipDim(pl.srcW, pl.halvings) > t.width || mipDim(pl.srcH, pl.halvings) > t.height))
            pl.halvings++;
        pl.temp = (int)nextTemp;
        size_t &sc = t.format == PTX_TEXTURE_RGBA32F ? plan.scratchF : plan.scratch8;
        sc = std::max(sc, chainTexels(pl.srcW, pl.srcH, pl.halvings + 1));
    }
    return PTX_OK;
}

// The alpha footprint table of a scene with non-opaque geometry: one entry per colour texture of some material.
static int planAlphaFootprints(PtxRenderer *r, const PtxSceneDesc *s, TexturePlan &plan)
{
    auto mark = [&](uint32_t colorIdx) {
        if (colorIdx < PTX_SCENE_TEXTURE_OFFSET || colorIdx - PTX_SCENE_TEXTURE_OFFSET >= plan.textureCount)
            return;
        const uint32_t ti = colorIdx - PTX_SCENE_TEXTURE_OFFSET;
        if (plan.alphaTexOf[ti] != kNoAlphaTex)
            return;
        plan.alphaTexOf[ti] = (uint32_t)plan.alphaTex.size();
        plan.alphaTex.push_back({ plan.table[ti].width, plan.table[ti].height, (uint32_t)plan.alphaQuads, 0u });
        plan.alphaQuads += (size_t)plan.table[ti].width * plan.table[ti].height;
    };
    for (uint32_t i = 0; i < s->metallicRoughnessMaterialCount; i++) mark(s->metallicRoughnessMaterials[i].ColorIdx);
    for (uint32_t i = 0; i < s->specularGlossinessMaterialCount; i++) mark(s->specularGlossinessMaterials[i].ColorIdx);
    for (uint32_t i = 0; i < s->phongMaterialCount; i++) mark(s->phongMaterials[i].ColorIdx);
    // The extent of an alpha texture rides in 15 + 15 bits of the triangle record.  Unreachable as long as placeSceneTexture
    // scales every scene texture to at most maxExtent <= 4096 on a side; kept for the day that limit is raised.
    for (const AlphaTex &at : plan.alphaTex)
        if (at.width > 32768u || at.height > 32768u)
            return fail(r, PTX_ERROR_INVALID_ARGUMENT, "a colour texture of a non-opaque geometry is larger than 32768 texels across");
    if (plan.alphaQuads >= 0xffffffffull)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "alpha footprints exceed 2^32 texels");
    return PTX_OK;
}

// Stage 3 (row N1): where every texel of every texture goes.  deviceTotalBytes: read for the default budget only.
static int planTextures(PtxRenderer *r, const PtxSceneDesc *s, uint64_t deviceTotalBytes, bool anyNonOpaque, TexturePlan &plan)
{
    int rc;
    plan.textureCount = s->textures ? s->textureCount : 0;
    plan.skyKind = s->skybox ? s->skyboxKind : (uint32_t)PTX_SKYBOX_CLEAR_COLOR;
    if (plan.skyKind > PTX_SKYBOX_CUBE)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "unknown skybox kind %u", plan.skyKind);
    plan.total = plan.textureCount + (plan.skyKind == PTX_SKYBOX_2D ? 1u : plan.skyKind == PTX_SKYBOX_CUBE ? 6u : 0u);
    if (plan.skyKind == PTX_SKYBOX_CUBE)
        for (uint32_t f = 0; f < 6; f++)
            if (s->skybox[f].width != s->skybox[0].width || s->skybox[f].height != s->skybox[0].width || s->skybox[f].format != s->skybox[0].format)
                return fail(r, PTX_ERROR_INVALID_ARGUMENT, "cube skybox: the six faces must be equal squares of one format");
    uint32_t maxExtent[kTextureFormats];
    maxTextureExtents(s, plan.textureCount, deviceTotalBytes, maxExtent);
    plan.place.resize(plan.total);
    plan.table.resize(plan.total);
    uint32_t scaled = 0;
    for (uint32_t i = 0; i < plan.total; i++)
    {
        const PtxTextureDesc &d = textureDescOf(s, plan.textureCount, i);
        DevTexture &t = plan.table[i];
        Placement &pl = plan.place[i];
        if (d.format >= kTextureFormats)
            return fail(r, PTX_ERROR_INVALID_ARGUMENT, "texture %u: unknown format %u", i, d.format);
        if (isBcFormat(d.format) && i >= plan.textureCount) // the reference loads its skyboxes through stb only
            return fail(r, PTX_ERROR_INVALID_ARGUMENT, "skybox image %u: block-compressed format %u", i - plan.textureCount, d.format);
        pl = { d.width ? d.width : 1, d.height ? d.height : 1, d.levels ? d.levels : 1u, 0u, false, 0u, -1 };
        t = { pl.srcW, pl.srcH, 1u, d.format, {} };
        if (isBcFormat(d.format))
        {
            if ((rc = placeBcTexture(r, i, maxExtent[d.format], t, pl)) != PTX_OK) return rc;
            if (pl.rejected)
                plan.rejected.push_back(i); // (the white texel: no sampler needed on its account)
            else
            {
                plan.samplerNeeded = true;
                pl.bcOffset = plan.bcBytes;
                plan.bcBytes += (bcChainBytes(t.width, t.height, 0, t.levels, t.format) + 15u) & ~(size_t)15u;
                plan.nbc = placeLevels(t, plan.nbc);
                if (plan.nbc > 0xffffffffull)
                    return fail(r, PTX_ERROR_INVALID_ARGUMENT, "texture pool exceeds 2^32 texels");
                continue;
            }
        }
        else if (i < plan.textureCount)
        {
            if ((rc = placeSceneTexture(r, i, maxExtent[d.format], plan.total + scaled, t, pl, plan)) != PTX_OK) return rc;
            scaled += pl.temp >= 0 ? 1u : 0u;
            // A 1x1 opaque-white 8-bit texture decodes to exactly (1,1,1,1) in both formats, which is what the
            // kernels without the sampler return for any index >= 9: only other content needs the TEX variants.
            plan.samplerNeeded |= !(t.width == 1 && t.height == 1 && d.format != PTX_TEXTURE_RGBA32F && d.data &&
                                    *static_cast<const uint32_t *>(d.data) == 0xffffffffu && pl.srcW == 1 && pl.srcH == 1);
        }
        size_t &cursor = t.format == PTX_TEXTURE_RGBA32F ? plan.nf : plan.n8;
        cursor = placeLevels(t, cursor);
    }
    // scratch chains of the textures that are scaled down: one region per pool behind the textures, used by one
    // texture after the other (stream order); their table entries follow the real ones
    plan.table.resize(plan.total + scaled);
    for (uint32_t i = 0; i < plan.total; i++)
        if (plan.place[i].temp >= 0)
        {
            DevTexture &t = plan.table[(size_t)plan.place[i].temp];
            t = { plan.place[i].srcW, plan.place[i].srcH, plan.place[i].halvings + 1, plan.table[i].format, {} };
            placeLevels(t, t.format == PTX_TEXTURE_RGBA32F ? plan.nf : plan.n8);
        }
    // (the second sum is the pool the render kernels sample, uploadTextures)
    if (plan.n8 + plan.scratch8 > 0xffffffffull || plan.nf + plan.scratchF > 0xffffffffull || (uint64_t)plan.nf + plan.n8 + plan.nbc > 0xffffffffull)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "texture pool exceeds 2^32 texels");
    plan.renderTable.assign(plan.table.begin(), plan.table.begin() + plan.total);
    for (DevTexture &t : plan.renderTable)
        if (isBcFormat(t.format))
            placeLevels(t, plan.nf + plan.n8 + t.levelOffset[0]);
        else if (t.format != PTX_TEXTURE_RGBA32F)
            placeLevels(t, plan.nf + t.levelOffset[0]);
    plan.alphaTexOf.assign(plan.textureCount ? plan.textureCount : 1u, kNoAlphaTex);
    return anyNonOpaque ? planAlphaFootprints(r, s, plan) : PTX_OK;
}

// Stage 4: the bind-pose vertices, the indices, the animated arrays, the materials, the pairs; the scene's counts and flags.
static int uploadGeometry(PtxRenderer *r, const PtxSceneDesc *s, FlatScene &flat)
{
    SceneData &sc = r->scene;
    int rc;
    sc.pairCount = static_cast<uint32_t>(flat.pairs.size()); sc.triCount = static_cast<uint32_t>(flat.triangles);
    sc.anyNonOpaque = flat.anyNonOpaque; sc.mixedMaterialTypes = flat.mixedMaterialTypes; sc.mixedTextured = flat.mixedTextured;
    sc.hostPairs = flat.pairs; sc.pairInstance = std::move(flat.pairInstance); sc.pairMeshTransform = std::move(flat.pairMeshTransform);
    sc.hostDebugPairs = flat.debugPairs;
    sc.instanceCount = s->instanceCount; sc.staticVertexCount = s->vertexCount; sc.dxNormalTextures = s->dxNormalTextures;
    sc.skinnedCount = static_cast<uint32_t>(flat.skinSource.size()); sc.boneCount = 0;
    // bind pose of every skinned copy (OutBindPoseAnimatedVertices)
    flat.verts.assign(s->vertices, s->vertices + s->vertexCount);
    flat.verts.reserve(flat.verts.size() + flat.skinSource.size());
    for (uint32_t src : flat.skinSource)
    {
        const PtxAnimatedVertex &a = s->animatedVertices[src];
        PtxVertex v;
        std::memset(&v, 0, sizeof(v));
        std::memcpy(v.Position, a.Position, 12); std::memcpy(v.TexCoords, a.TexCoords, 8); std::memcpy(v.Normal, a.Normal, 12);
        std::memcpy(v.Tangent, a.Tangent, 12); std::memcpy(v.Bitangent, a.Bitangent, 12);
        flat.verts.push_back(v);
    }
    flat.inds.assign(s->indices, s->indices + s->indexCount);
    if (s->animatedIndices)
        flat.inds.insert(flat.inds.end(), s->animatedIndices, s->animatedIndices + s->animatedIndexCount);
    if ((rc = upload(r, sc.vertices, flat.verts.data(), flat.verts.size())) != PTX_OK) return rc;
    if ((rc = upload(r, sc.indices, flat.inds.data(), flat.inds.size())) != PTX_OK) return rc;
    if ((rc = upload(r, sc.animatedVertices, s->animatedVertices, flat.skinSource.empty() ? 0 : s->animatedVertexCount)) != PTX_OK) return rc;
    if ((rc = upload(r, sc.skinSource, flat.skinSource.data(), flat.skinSource.size())) != PTX_OK) return rc;
    if ((rc = upload(r, sc.mr, s->metallicRoughnessMaterials, s->metallicRoughnessMaterialCount)) != PTX_OK) return rc;
    if ((rc = upload(r, sc.sg, s->specularGlossinessMaterials, s->specularGlossinessMaterialCount)) != PTX_OK) return rc;
    if ((rc = upload(r, sc.phong, s->phongMaterials, s->phongMaterialCount)) != PTX_OK) return rc;
    if ((rc = upload(r, sc.pairs, flat.pairs.data(), flat.pairs.size())) != PTX_OK) return rc;
    if ((rc = upload(r, sc.debugPairs, flat.debugPairs.data(), flat.debugPairs.size())) != PTX_OK) return rc;
    return upload(r, sc.pairFirst, flat.pairFirst.data(), flat.pairFirst.size());
}

// k_decode_bc for texture `t` (the plan's entry; `rt` its entry of the render table): every level in one launch, from the kept
// levels' blocks at `blocks` into the texture's region of the decoded pool.  rows: the one-thread-per-block-row mapping.
static void decodeBcTexture(const DevTexture &t, const DevTexture &rt, const uint8_t *blocks, const float *srgbLut, float4 *decoded, bool rows, hipStream_t stream)
{
    BcDecodeArgs a = {};
    a.width = t.width; a.height = t.height; a.levels = t.levels;
    for (uint32_t l = 0; l < 16u; l++)
    {
        a.itemFirst[l] = 0xffffffffu;
        if (l >= t.levels)
            continue;
        const uint32_t w = mipDim(t.width, l), h = mipDim(t.height, l);
        a.itemFirst[l] = a.items;
        a.items += (rows ? (w + 3u) / 4u : w) * h;
        a.blockFirst[l] = (uint32_t)bcChainBytes(t.width, t.height, 0, l, t.format);
        a.decodedFirst[l] = rt.levelOffset[l];
    }
    const uint32_t grid = (a.items + 255u) / 256u;
#define PT_BC_LAUNCH(F)                                                                        \
    case F:                                                                                    \
        if (rows) k_decode_bc<F, true><<<grid, 256, 0, stream>>>(a, blocks, srgbLut, decoded); \
        else k_decode_bc<F, false><<<grid, 256, 0, stream>>>(a, blocks, srgbLut, decoded);     \
        break;
    switch (t.format)
    {
        PT_BC_LAUNCH(PTX_TEXTURE_BC1_UNORM)
        PT_BC_LAUNCH(PTX_TEXTURE_BC1_SRGB)
        PT_BC_LAUNCH(PTX_TEXTURE_BC3_SRGB)
        PT_BC_LAUNCH(PTX_TEXTURE_BC5_UNORM)
    default: break;
    }
#undef PT_BC_LAUNCH
}

// Stage 5 (row N1): every texture into the pools of the upload formats -- the file's own chain, or its level 0 (scaled through the
// scratch chain where the plan says so) and the mip chain below it level by level on the device --, then decoded into the pool the
// render kernels sample.  The upload-format pools are this stage's own: freed when it returns, whichever way (hipFree waits).
// extraTexels: room behind the decoded pool (the stand-in texels of a streamed upload).
static int uploadTextures(PtxRenderer *r, const PtxSceneDesc *s, const TexturePlan &plan, size_t extraTexels = 0)
{
    SceneData &sc = r->scene;
    DevBuf<DevTexture> textures; // upload time only: the table, the pools of the image formats in which mip chains are built,
    DevBuf<uint32_t> texels8;    // the sRGB byte -> linear table
    DevBuf<float4> texelsF;
    DevBuf<float> srgbLut;
    DevBuf<uint8_t> bcBlocks;    // the kept levels of the block-compressed textures, as the files hold them
    HIP_TRY(r, srgbLut.alloc(256));
    k_build_srgb_lut<<<1, 256, 0, r->stream>>>(srgbLut.p);
    sc.rejectedTextures = plan.rejected;
    sc.textureCount = plan.textureCount; sc.skyKind = plan.skyKind; sc.samplerNeeded = plan.samplerNeeded;
    HIP_TRY(r, textures.alloc(plan.table.size()));
    HIP_TRY(r, texels8.alloc(plan.n8 + plan.scratch8));
    HIP_TRY(r, texelsF.alloc(plan.nf + plan.scratchF));
    if (plan.n8)
        HIP_TRY(r, hipMemsetAsync(texels8.p, 0, plan.n8 * 4, r->stream)); // a texture without data reads as zeros
    if (plan.nf)
        HIP_TRY(r, hipMemsetAsync(texelsF.p, 0, plan.nf * 16, r->stream));
    if (!plan.table.empty())
        HIP_TRY(r, hipMemcpyAsync(textures.p, plan.table.data(), plan.table.size() * sizeof(DevTexture), hipMemcpyHostToDevice, r->stream));
    const TextureView tv = { textures.p, plan.textureCount, texels8.p, texelsF.p, srgbLut.p };
    for (uint32_t i = 0; i < plan.total; i++)
    {
        const PtxTextureDesc &d = textureDescOf(s, plan.textureCount, i);
        const DevTexture &t = plan.table[i];
        const Placement &pl = plan.place[i];
        const bool isFloat = t.format == PTX_TEXTURE_RGBA32F;
        const size_t texel = isFloat ? 16 : 4;
        if (isBcFormat(t.format)) // never in the 8-bit pool: decoded below, straight from its blocks
            continue;
        const void *data = textureData(d, pl); // (a rejected texture: its one white texel, whatever the caller passed)
        auto poolAt = [&](uint32_t offset) -> void * { return isFloat ? (void *)(texelsF.p + offset) : (void *)(texels8.p + offset); };
        auto blit = [&](uint32_t src, uint32_t srcLevel, uint32_t dst, uint32_t dstLevel) {
            const uint32_t dw = mipDim(plan.table[dst].width, dstLevel), dh = mipDim(plan.table[dst].height, dstLevel);
            k_blit_level<<<(dw * dh + 255) / 256, 256, 0, r->stream>>>(tv, src, srcLevel, dst, dstLevel, texels8.p, texelsF.p);
        };
        if (d.data && pl.useFileChain)
        {
            // the file's own levels, from the one that has the budgeted extent
            const uint8_t *p = static_cast<const uint8_t *>(d.data) + chainTexels(pl.srcW, pl.srcH, pl.firstFile) * texel;
            for (uint32_t l = 0; l < t.levels; l++)
                HIP_TRY(r, hipMemcpyAsync(poolAt(t.levelOffset[l]), p + chainTexels(t.width, t.height, l) * texel,
                                          (size_t)mipDim(t.width, l) * mipDim(t.height, l) * texel, hipMemcpyHostToDevice, r->stream));
            continue;
        }
        if (d.data && pl.temp >= 0)
        {
            // scaled down: the file's level 0 into the scratch chain, halved by linear blits, then into level 0
            const DevTexture &tt = plan.table[(size_t)pl.temp];
            HIP_TRY(r, hipMemcpyAsync(poolAt(tt.levelOffset[0]), d.data, (size_t)pl.srcW * pl.srcH * texel, hipMemcpyHostToDevice, r->stream));
            for (uint32_t l = 1; l <= pl.halvings; l++)
                blit((uint32_t)pl.temp, l - 1, (uint32_t)pl.temp, l);
            if (mipDim(pl.srcW, pl.halvings) == t.width && mipDim(pl.srcH, pl.halvings) == t.height)
                HIP_TRY(r, hipMemcpyAsync(poolAt(t.levelOffset[0]), poolAt(tt.levelOffset[pl.halvings]), (size_t)t.width * t.height * texel,
                                          hipMemcpyDeviceToDevice, r->stream));
            else
                blit((uint32_t)pl.temp, pl.halvings, i, 0);
        }
        else if (data)
            HIP_TRY(r, hipMemcpyAsync(poolAt(t.levelOffset[0]), data, (size_t)t.width * t.height * texel, hipMemcpyHostToDevice, r->stream));
        for (uint32_t l = 1; l < t.levels; l++)
            blit(i, l - 1, i, l);
    }
    // The pool the render kernels sample (pt_device.hpp, fetchTexel): every level of every texture decoded to four floats,
    // the RGBA32F pool first, the 8-bit textures behind it; `renderTextures` is the table with offsets into that pool.
    // the block-compressed textures behind both, decoded by k_decode_bc from the block pool
    HIP_TRY(r, sc.renderTexels.alloc(plan.nf + plan.n8 + plan.nbc + extraTexels));
    HIP_TRY(r, sc.renderTextures.alloc(plan.total));
    if (plan.nf)
        HIP_TRY(r, hipMemcpyAsync(sc.renderTexels.p, texelsF.p, plan.nf * sizeof(float4), hipMemcpyDeviceToDevice, r->stream));
    for (uint32_t i = 0; i < plan.total; i++)
    {
        const DevTexture &t = plan.table[i];
        if (t.format == PTX_TEXTURE_RGBA32F || isBcFormat(t.format))
            continue;
        const size_t count = chainTexels(t.width, t.height, t.levels);
        const uint32_t first = t.levelOffset[0];
        k_decode_texels<<<(uint32_t)((count + 255) / 256), 256, 0, r->stream>>>(texels8.p, srgbLut.p, first, (uint32_t)count, t.format,
                                                                              sc.renderTexels.p + plan.nf + first);
    }
    if (plan.nbc)
    {
        // only the levels that are kept, straight from the caller's data; one launch per texture
        HIP_TRY(r, bcBlocks.alloc(plan.bcBytes));
        for (uint32_t i = 0; i < plan.textureCount; i++)
        {
            const DevTexture &t = plan.table[i], &rt = plan.renderTable[i];
            const Placement &pl = plan.place[i];
            if (!isBcFormat(t.format))
                continue;
            const size_t count = chainTexels(t.width, t.height, t.levels);
            if (!s->textures[i].data) // a texture without data reads as zeros (a pending one: until its upload)
            {
                HIP_TRY(r, hipMemsetAsync(sc.renderTexels.p + rt.levelOffset[0], 0, count * sizeof(float4), r->stream));
                continue;
            }
            const uint8_t *src = static_cast<const uint8_t *>(s->textures[i].data) + bcChainBytes(pl.srcW, pl.srcH, 0, pl.firstFile, t.format);
            HIP_TRY(r, hipMemcpyAsync(bcBlocks.p + pl.bcOffset, src, bcChainBytes(t.width, t.height, 0, t.levels, t.format), hipMemcpyHostToDevice, r->stream));
            decodeBcTexture(t, rt, bcBlocks.p + pl.bcOffset, srgbLut.p, sc.renderTexels.p, r->env.bcRowMapping, r->stream);
        }
    }
    if (plan.total)
        HIP_TRY(r, hipMemcpyAsync(sc.renderTextures.p, plan.renderTable.data(), plan.total * sizeof(DevTexture), hipMemcpyHostToDevice, r->stream));
    HIP_TRY(r, hipStreamSynchronize(r->stream)); // the caller's texel arrays may go away, and the pools of the upload formats do
    HIP_TRY(r, hipGetLastError());
    return PTX_OK;
}

// Stage 6: what the any-hit stages read of the textures.
// pending / extraQuads (a streamed upload): the textures whose texels are still to come get their quads from
// ptx_texture_upload, and the stand-in quads sit behind the scene's.
static int alphaFootprints(PtxRenderer *r, const TexturePlan &plan, const std::vector<uint8_t> *pending = nullptr, size_t extraQuads = 0)
{
    SceneData &sc = r->scene;
    int rc;
    if (sc.anyNonOpaque)
        HIP_TRY(r, sc.alphaQuads.alloc(plan.alphaQuads + extraQuads));
    for (uint32_t ti = 0; ti < plan.textureCount; ti++)
        if (plan.alphaTexOf[ti] != kNoAlphaTex && !(pending && (*pending)[ti]))
        {
            const AlphaTex &at = plan.alphaTex[plan.alphaTexOf[ti]];
            k_alpha_quads<<<(at.width * at.height + 255) / 256, 256, 0, r->stream>>>(at.width, at.height, sc.renderTexels.p + plan.renderTable[ti].levelOffset[0],
                                                                                    sc.alphaQuads.p + at.offset);
        }
    if ((rc = upload(r, sc.alphaTex, plan.alphaTex.data(), plan.alphaTex.size())) != PTX_OK) return rc;
    return upload(r, sc.alphaTexOf, plan.alphaTexOf.data(), plan.alphaTexOf.size());
}

// ---- streamed textures: ptx_scene_upload_streamed, ptx_texture_upload, ptx_textures_commit, ptx_texture_residency ----------------
// A texture of a streamed upload is PENDING (no texels yet: its table entries name the 1 x 1 stand-in), UPLOADED (its pool
// region is being filled on the upload stream; the tables still name the stand-in) or RESIDENT (committed, or it came with
// its data).  Nothing a frame reads changes outside ptx_textures_commit.
enum : uint8_t { kTexResident = 0, kTexPending = 1, kTexUploaded = 2 };
constexpr uint32_t kStreamRing = 2; // staging slots: a ptx_texture_upload waits only when both still hold an upload in flight

struct TextureStreaming
{
    int device = 0;
    TexturePlan plan;
    std::vector<PtxTextureDesc> declared; // width / height / format / levels as ptx_scene_upload_streamed saw them
    std::vector<uint8_t> state;           // [textureCount] kTex*
    uint32_t pendingCount = 0, uploadedCount = 0;
    uint32_t standInTexel = 0, standInQuad = 0; // first of the nine stand-ins in renderTexels / alphaQuads
    std::vector<DevTexture> liveTable;    // what the device tables hold for the pending textures at upload
    std::vector<AlphaTex> liveAlphaTex;
    DevBuf<DevTexture> finalTextures;     // the plan's entries, for k_commit_textures
    DevBuf<AlphaTex> finalAlphaTex;
    DevBuf<float> srgbLut;
    hipStream_t stream = nullptr;         // the upload stream, created by the first ptx_texture_upload
    hipEvent_t evUploaded = nullptr, evCommitted = nullptr;
    uint32_t *commitList = nullptr;       // pinned, [textureCount]: every texture is committed once, so entries are never reused
    uint32_t commitCursor = 0;
    uint64_t commits = 0;                 // commits that switched something: borrowers' streams wait for evCommitted
    struct Slot
    {
        void *host = nullptr;             // pinned: the slot's one-texture table (two entries), then the caller's texels
        size_t hostBytes = 0;
        DevBuf<uint8_t> pool;             // device: the one-texture pool of the image format (chain, then the scratch chain)
        DevBuf<DevTexture> table;
        hipEvent_t done = nullptr;
        bool busy = false;
    } ring[kStreamRing];
    uint32_t nextSlot = 0;
    ~TextureStreaming()
    {
        (void)hipSetDevice(device);
        if (stream)
        {
            (void)hipStreamSynchronize(stream);
            (void)hipStreamDestroy(stream);
        }
        for (Slot &sl : ring)
        {
            if (sl.host) (void)hipHostFree(sl.host);
            if (sl.done) (void)hipEventDestroy(sl.done);
        }
        if (commitList) (void)hipHostFree(commitList);
        if (evUploaded) (void)hipEventDestroy(evUploaded);
        if (evCommitted) (void)hipEventDestroy(evCommitted);
    }
};

// Frames, rays and lookups enqueued after a commit see it: on the owner by stream order (the commit is enqueued on its render
// stream), on a borrower by this wait.
static int waitForCommits(PtxRenderer *r)
{
    if (!r->link.owner)
        return PTX_OK;
    const TextureStreaming *st = r->link.owner->scene.streaming.get();
    if (st && st->commits)
        HIP_TRY(r, hipStreamWaitEvent(r->stream, st->evCommitted, 0));
    return PTX_OK;
}

// The streamed half of an upload, behind uploadTextures and alphaFootprints: stand-ins, the tables of the pending textures.
static int beginStreaming(PtxRenderer *r, const PtxSceneDesc *s, std::shared_ptr<TextureStreaming> st, const uint32_t *standIn)
{
    SceneData &sc = r->scene;
    const TexturePlan &plan = st->plan;
    int rc;
    st->device = r->device;
    st->standInTexel = (uint32_t)(plan.nf + plan.n8 + plan.nbc);
    st->standInQuad = (uint32_t)plan.alphaQuads;
    HIP_TRY(r, st->srgbLut.alloc(256));
    k_build_srgb_lut<<<1, 256, 0, r->stream>>>(st->srgbLut.p);
    k_stream_stand_ins<<<1, 64, 0, r->stream>>>(sc.renderTexels.p + st->standInTexel, sc.anyNonOpaque ? sc.alphaQuads.p + st->standInQuad : nullptr);
    st->liveTable = plan.renderTable;
    st->liveAlphaTex = plan.alphaTex;
    for (uint32_t i = 0; i < plan.textureCount; i++)
    {
        st->declared[i] = s->textures[i];
        st->declared[i].data = nullptr;
        if (st->state[i] != kTexPending)
            continue;
        const uint32_t k = standIn ? standIn[i] : (uint32_t)PTX_PLACEHOLDER_TEXTURE_INDEX;
        st->liveTable[i] = { 1u, 1u, 1u, plan.renderTable[i].format, { st->standInTexel + k } };
        if (plan.alphaTexOf[i] != kNoAlphaTex)
            st->liveAlphaTex[plan.alphaTexOf[i]] = { 1u, 1u, st->standInQuad + k, 0u };
    }
    if (plan.total)
        HIP_TRY(r, hipMemcpyAsync(sc.renderTextures.p, st->liveTable.data(), plan.total * sizeof(DevTexture), hipMemcpyHostToDevice, r->stream));
    if (!st->liveAlphaTex.empty())
        HIP_TRY(r, hipMemcpyAsync(sc.alphaTex.p, st->liveAlphaTex.data(), st->liveAlphaTex.size() * sizeof(AlphaTex), hipMemcpyHostToDevice, r->stream));
    if ((rc = upload(r, st->finalTextures, plan.renderTable.data(), plan.total)) != PTX_OK) return rc;
    if ((rc = upload(r, st->finalAlphaTex, plan.alphaTex.data(), plan.alphaTex.size())) != PTX_OK) return rc;
    HIP_TRY(r, hipHostMalloc(reinterpret_cast<void **>(&st->commitList), (plan.textureCount ? plan.textureCount : 1u) * sizeof(uint32_t), hipHostMallocDefault));
    HIP_TRY(r, hipEventCreateWithFlags(&st->evUploaded, hipEventDisableTiming));
    HIP_TRY(r, hipEventCreateWithFlags(&st->evCommitted, hipEventDisableTiming));
    sc.streaming = st;
    return PTX_OK;
}

static int sceneUpload(PtxRenderer *r, const PtxSceneDesc *s, bool streamed = false, const uint32_t *standIn = nullptr)
{
    const char *who = streamed ? "ptx_scene_upload_streamed" : "ptx_scene_upload";
    if (!r || !s)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "%s: null argument", who);
    HIP_TRY(r, hipSetDevice(r->device));
    // The plan: host only.  A description that is refused here leaves the handle as it was -- its own scene, or the one it
    // borrows -- and nothing below refuses one.
    int rc;
    FlatScene flat;
    std::shared_ptr<TextureStreaming> st;
    TexturePlan localPlan;
    if (streamed)
        st = std::make_shared<TextureStreaming>();
    TexturePlan &plan = streamed ? st->plan : localPlan;
    size_t freeB = 0, totalB = 0;
    if ((rc = validateSceneDesc(r, s)) != PTX_OK) return rc;
    if ((rc = flattenScene(r, s, flat)) != PTX_OK) return rc;
    if (!s->forceFullTextureSize && s->textures && s->textureCount && !s->textureMemoryBudget) // the one case planTextures reads it in
        HIP_TRY(r, hipMemGetInfo(&freeB, &totalB));
    if ((rc = planTextures(r, s, totalB, flat.anyNonOpaque, plan)) != PTX_OK) return rc;
    if (streamed)
    {
        st->state.assign(plan.textureCount, kTexResident);
        st->declared.resize(plan.textureCount);
        for (uint32_t i = 0; i < plan.textureCount; i++)
        {
            if (standIn && standIn[i] >= PTX_SCENE_TEXTURE_OFFSET)
                return fail(r, PTX_ERROR_INVALID_ARGUMENT, "%s: stand-in %u of texture %u is not one of the nine fixed textures", who, standIn[i], i);
            if (!s->textures[i].data && !plan.place[i].rejected) // (a rejected texture is its white texel: resident at once)
            {
                st->state[i] = kTexPending;
                st->pendingCount++;
            }
        }
        if ((uint64_t)plan.nf + plan.n8 + plan.nbc + PTX_SCENE_TEXTURE_OFFSET > 0xffffffffull || (uint64_t)plan.alphaQuads + PTX_SCENE_TEXTURE_OFFSET >= 0xffffffffull)
            return fail(r, PTX_ERROR_INVALID_ARGUMENT, "%s: texture pool exceeds 2^32 texels", who);
    }

    // from here on the old scene is gone, whatever happens
    detachSharedScene(r); // a renderer that was borrowing a scene gets its own again
    quiesceSharers(r);
    r->scene.streaming.reset(); // (waits for the uploads that still write into the old pools)
    r->link.ready = r->accel.ready = false;
    r->link.epoch++;
    r->accel.build = BuildState();
    // the pose bookkeeping starts over: tracking off, no snapshot, and a serial that no history of the old scene leads back to
    r->scene.pose.release();
    r->scene.pose.enabled = false;
    r->scene.pose.serial += 2;
    // ... and this handle's own guides and history (made on the old scene, or on an owner's with serials of its own) to no pose at all
    r->chain.status.sceneChanged();
    if ((rc = uploadGeometry(r, s, flat)) != PTX_OK) return rc;
    if ((rc = uploadTextures(r, s, plan, streamed ? PTX_SCENE_TEXTURE_OFFSET : 0)) != PTX_OK) return rc;
    if ((rc = alphaFootprints(r, plan, streamed ? &st->state : nullptr, streamed ? PTX_SCENE_TEXTURE_OFFSET : 0)) != PTX_OK) return rc;
    if (streamed && (rc = beginStreaming(r, s, st, standIn)) != PTX_OK) return rc;
    HIP_TRY(r, hipStreamSynchronize(r->stream)); // `flat`, `plan` and the caller's arrays may go away
    if (streamed)
        HIP_TRY(r, hipGetLastError());
    r->link.ready = true;
    r->stats.triangles = flat.triangles;
    return PTX_OK;
}

static int streamingOf(PtxRenderer *r, const char *who, TextureStreaming **out)
{
    if (!r)
        return PTX_ERROR_INVALID_ARGUMENT;
    if (r->link.owner)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "%s: this renderer shares another renderer's scene (ptx_share_scene); uploads are the owner's calls", who);
    if (!r->link.ready)
        return fail(r, PTX_ERROR_NOT_READY, "%s: no scene uploaded", who);
    if (!r->scene.streaming)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "%s: the scene was not uploaded by ptx_scene_upload_streamed", who);
    *out = r->scene.streaming.get();
    return PTX_OK;
}

// The chain of texture `i` below its level 0, which sits encoded at the head of the slot's pool: k_stream_chain while every
// extent of the level above is even or 1, k_blit_level from there on; everything decoded into the texture's region of
// renderTexels.  levelwise: k_blit_level for every level (PTX_STREAM_LEVELWISE, and what the blocking upload does).
static int streamChain(PtxRenderer *r, TextureStreaming *st, TextureStreaming::Slot &sl, uint32_t i, const TextureView &tv, bool levelwise)
{
    const DevTexture &t = st->plan.table[i], &rt = st->plan.renderTable[i];
    const bool isFloat = t.format == PTX_TEXTURE_RGBA32F;
    const uint32_t logTile = isFloat ? kStreamSteps - 1 : kStreamSteps, tile = 1u << logTile;
    float4 *decoded = r->scene.renderTexels.p;
    auto even = [&](uint32_t l) {
        const uint32_t w = mipDim(t.width, l), h = mipDim(t.height, l);
        return l + 1 < t.levels && (w % 2 == 0 || w == 1) && (h % 2 == 0 || h == 1);
    };
    uint32_t cur = 0;       // the coarsest level the pool holds encoded
    uint32_t firstToDecode = 0; // levels below this one are in renderTexels already
    while (!levelwise && even(cur))
    {
        StreamChainArgs a = {};
        while (a.steps < logTile && even(cur + a.steps))
            a.steps++;
        a.srcOffset = (uint32_t)chainTexels(t.width, t.height, cur);
        a.sw = mipDim(t.width, cur); a.sh = mipDim(t.height, cur);
        a.format = t.format;
        a.writeSource = cur == 0 ? 1u : 0u;
        a.encOut = cur + a.steps + 1 < t.levels ? (uint32_t)chainTexels(t.width, t.height, cur + a.steps) : 0xffffffffu;
        for (uint32_t k = 0; k <= a.steps; k++)
            a.decoded[k] = rt.levelOffset[cur + k];
        const uint32_t grid = ((a.sw + tile - 1) / tile) * ((a.sh + tile - 1) / tile);
        if (isFloat)
            k_stream_chain<true><<<grid, kStreamBlock, 0, st->stream>>>(a, sl.pool.p, st->srgbLut.p, decoded);
        else
            k_stream_chain<false><<<grid, kStreamBlock, 0, st->stream>>>(a, sl.pool.p, st->srgbLut.p, decoded);
        cur += a.steps;
        firstToDecode = cur + 1;
    }
    for (uint32_t l = cur + 1; l < t.levels; l++)
    {
        const uint32_t dw = mipDim(t.width, l), dh = mipDim(t.height, l);
        k_blit_level<<<(dw * dh + 255) / 256, 256, 0, st->stream>>>(tv, 0u, l - 1, 0u, l, reinterpret_cast<uint32_t *>(sl.pool.p), reinterpret_cast<float4 *>(sl.pool.p));
    }
    if (firstToDecode < t.levels)
    {
        const size_t first = chainTexels(t.width, t.height, firstToDecode), count = chainTexels(t.width, t.height, t.levels) - first;
        if (isFloat)
            HIP_TRY(r, hipMemcpyAsync(decoded + rt.levelOffset[firstToDecode], reinterpret_cast<float4 *>(sl.pool.p) + first, count * sizeof(float4),
                                      hipMemcpyDeviceToDevice, st->stream));
        else
            k_decode_texels<<<(uint32_t)((count + 255) / 256), 256, 0, st->stream>>>(reinterpret_cast<uint32_t *>(sl.pool.p), st->srgbLut.p, (uint32_t)first, (uint32_t)count,
                                                                                    t.format, decoded + rt.levelOffset[firstToDecode]);
    }
    return PTX_OK;
}

// TextureUploader's submit thread for one texture (TextureUploader.cpp:312-360): the caller's texels into a staging slot, the
// device work on the upload stream.  Nothing a frame reads is touched.
static int textureUpload(PtxRenderer *r, uint32_t index, const PtxTextureDesc *d)
{
    const char *who = "ptx_texture_upload";
    TextureStreaming *st = nullptr;
    int rc;
    if ((rc = streamingOf(r, who, &st)) != PTX_OK) return rc;
    const TexturePlan &plan = st->plan;
    if (!d || index >= plan.textureCount)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "%s: texture index %u out of range (%u textures)", who, index, plan.textureCount);
    const PtxTextureDesc &decl = st->declared[index];
    auto one = [](uint32_t v) { return v ? v : 1u; };
    if (one(d->width) != one(decl.width) || one(d->height) != one(decl.height) || d->format != decl.format || one(d->levels) != one(decl.levels))
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "%s: texture %u was declared %u x %u, format %u, %u level(s)", who, index, decl.width, decl.height, decl.format,
                    decl.levels);
    if (!d->data)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "%s: texture %u: null data", who, index);
    if (plan.place[index].rejected)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "%s: texture %u was rejected by the upload rules of its block-compressed format (ptx_textures_rejected)", who, index);
    if (st->state[index] != kTexPending)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "%s: texture %u is not pending (already uploaded or resident)", who, index);
    HIP_TRY(r, hipSetDevice(r->device));
    if (!st->stream)
        HIP_TRY(r, hipStreamCreateWithFlags(&st->stream, hipStreamNonBlocking));

    const DevTexture &t = plan.table[index];
    const Placement &pl = plan.place[index];
    const bool isFloat = t.format == PTX_TEXTURE_RGBA32F, isBc = isBcFormat(t.format);
    const size_t texel = isFloat ? 16 : 4;
    // the slot's one-texture pool: the chain at its head, the scratch chain of a scaled texture behind it
    DevTexture tab[2];
    tab[0] = t;
    size_t poolTexels = placeLevels(tab[0], 0);
    tab[1] = tab[0];
    if (pl.temp >= 0)
    {
        tab[1] = plan.table[(size_t)pl.temp];
        poolTexels = placeLevels(tab[1], poolTexels);
    }
    // (a block-compressed texture: the slot's pool holds the kept levels' blocks and nothing else)
    const uint8_t *src = static_cast<const uint8_t *>(d->data) +
                         (isBc ? bcChainBytes(pl.srcW, pl.srcH, 0, pl.firstFile, t.format) : pl.useFileChain ? chainTexels(pl.srcW, pl.srcH, pl.firstFile) * texel : 0);
    const size_t srcBytes = isBc ? bcChainBytes(t.width, t.height, 0, t.levels, t.format)
                                 : (pl.useFileChain ? chainTexels(t.width, t.height, t.levels) : (size_t)pl.srcW * pl.srcH) * texel;
    const size_t header = 256; // the table, and the texels 16-byte aligned behind it

    // a free slot: the reference's free-buffer semaphore
    TextureStreaming::Slot &sl = st->ring[st->nextSlot];
    if (!sl.done)
        HIP_TRY(r, hipEventCreateWithFlags(&sl.done, hipEventDisableTiming));
    if (sl.busy)
    {
        HIP_TRY(r, hipEventSynchronize(sl.done));
        sl.busy = false;
    }
    if (sl.hostBytes < header + srcBytes)
    {
        if (sl.host)
            (void)hipHostFree(sl.host);
        sl.host = nullptr;
        sl.hostBytes = 0;
        HIP_TRY(r, hipHostMalloc(&sl.host, header + srcBytes, hipHostMallocDefault));
        sl.hostBytes = header + srcBytes;
    }
    HIP_TRY(r, sl.pool.alloc(isBc ? srcBytes : poolTexels * texel));
    HIP_TRY(r, sl.table.alloc(2));
    st->nextSlot = (st->nextSlot + 1) % kStreamRing;
    std::memcpy(sl.host, tab, sizeof(tab));
    std::memcpy(static_cast<uint8_t *>(sl.host) + header, src, srcBytes);
    const uint8_t *staged = static_cast<const uint8_t *>(sl.host) + header;

    hipStream_t S = st->stream;
    float4 *decoded = r->scene.renderTexels.p;
    const DevTexture &rt = plan.renderTable[index];
    HIP_TRY(r, hipMemcpyAsync(sl.table.p, sl.host, sizeof(tab), hipMemcpyHostToDevice, S));
    const TextureView tv = { sl.table.p, 2u, reinterpret_cast<const uint32_t *>(sl.pool.p), reinterpret_cast<const float4 *>(sl.pool.p), st->srgbLut.p };
    auto poolAt = [&](uint32_t offset) -> void * { return sl.pool.p + (size_t)offset * texel; };
    auto blit = [&](uint32_t s0, uint32_t srcLevel, uint32_t d0, uint32_t dstLevel) {
        const uint32_t dw = mipDim(tab[d0].width, dstLevel), dh = mipDim(tab[d0].height, dstLevel);
        k_blit_level<<<(dw * dh + 255) / 256, 256, 0, S>>>(tv, s0, srcLevel, d0, dstLevel, reinterpret_cast<uint32_t *>(sl.pool.p), reinterpret_cast<float4 *>(sl.pool.p));
    };
    if (isBc)
    {
        // the kept levels' blocks: one copy, one launch into the texture's own region
        HIP_TRY(r, hipMemcpyAsync(sl.pool.p, staged, srcBytes, hipMemcpyHostToDevice, S));
        decodeBcTexture(t, rt, sl.pool.p, st->srgbLut.p, decoded, r->env.bcRowMapping, S);
    }
    else if (pl.useFileChain)
    {
        // the file's own levels from the one that has the budgeted extent: one copy, then decoded as they are
        const size_t count = chainTexels(t.width, t.height, t.levels);
        HIP_TRY(r, hipMemcpyAsync(sl.pool.p, staged, srcBytes, hipMemcpyHostToDevice, S));
        if (isFloat)
            HIP_TRY(r, hipMemcpyAsync(decoded + rt.levelOffset[0], sl.pool.p, srcBytes, hipMemcpyDeviceToDevice, S));
        else
            k_decode_texels<<<(uint32_t)((count + 255) / 256), 256, 0, S>>>(reinterpret_cast<uint32_t *>(sl.pool.p), st->srgbLut.p, 0u, (uint32_t)count, t.format,
                                                                           decoded + rt.levelOffset[0]);
    }
    else
    {
        if (pl.temp >= 0)
        {
            // scaled down: the file's level 0 into the scratch chain, halved by linear blits, then into level 0 (uploadTextures)
            HIP_TRY(r, hipMemcpyAsync(poolAt(tab[1].levelOffset[0]), staged, srcBytes, hipMemcpyHostToDevice, S));
            for (uint32_t l = 1; l <= pl.halvings; l++)
                blit(1, l - 1, 1, l);
            if (mipDim(pl.srcW, pl.halvings) == t.width && mipDim(pl.srcH, pl.halvings) == t.height)
                HIP_TRY(r, hipMemcpyAsync(poolAt(0), poolAt(tab[1].levelOffset[pl.halvings]), (size_t)t.width * t.height * texel, hipMemcpyDeviceToDevice, S));
            else
                blit(1, pl.halvings, 0, 0);
        }
        else
            HIP_TRY(r, hipMemcpyAsync(poolAt(0), staged, srcBytes, hipMemcpyHostToDevice, S));
        if ((rc = streamChain(r, st, sl, index, tv, r->env.streamLevelwise)) != PTX_OK) return rc;
    }
    if (plan.alphaTexOf[index] != kNoAlphaTex)
    {
        const AlphaTex &at = plan.alphaTex[plan.alphaTexOf[index]];
        k_alpha_quads<<<(at.width * at.height + 255) / 256, 256, 0, S>>>(at.width, at.height, decoded + rt.levelOffset[0], r->scene.alphaQuads.p + at.offset);
    }
    HIP_TRY(r, hipEventRecord(sl.done, S));
    HIP_TRY(r, hipGetLastError());
    sl.busy = true;
    st->state[index] = kTexUploaded;
    st->pendingCount--;
    st->uploadedCount++;
    return PTX_OK;
}

// Renderer::UpdateTexture (Renderer.cpp:441-471) for every texture uploaded so far: between frames, on the render stream.
static int texturesCommit(PtxRenderer *r, uint32_t *committed)
{
    const char *who = "ptx_textures_commit";
    TextureStreaming *st = nullptr;
    int rc;
    if (committed)
        *committed = 0;
    if ((rc = streamingOf(r, who, &st)) != PTX_OK) return rc;
    if (!st->uploadedCount)
        return PTX_OK;
    HIP_TRY(r, hipSetDevice(r->device));
    SceneData &sc = r->scene;
    const uint32_t first = st->commitCursor;
    bool alpha = false;
    for (uint32_t i = 0; i < st->plan.textureCount; i++)
        if (st->state[i] == kTexUploaded)
        {
            st->commitList[st->commitCursor++] = i;
            st->state[i] = kTexResident;
            alpha |= st->plan.alphaTexOf[i] != kNoAlphaTex;
        }
    const uint32_t n = st->commitCursor - first;
    st->uploadedCount = 0;
    // the uploads, then the switch: the render stream waits for the upload stream on the device, the host does not
    HIP_TRY(r, hipEventRecord(st->evUploaded, st->stream));
    HIP_TRY(r, hipStreamWaitEvent(r->stream, st->evUploaded, 0));
    quiesceSharers(r); // the borrowers' frames in flight still read the tables
    k_commit_textures<<<(n + 63) / 64, 64, 0, r->stream>>>(st->commitList + first, n, st->finalTextures.p, sc.renderTextures.p,
                                                          sc.anyNonOpaque ? sc.alphaTexOf.p : nullptr, st->finalAlphaTex.p, sc.alphaTex.p);
    if (alpha && sc.anyNonOpaque && r->accel.ready && r->accel.tree.slots) // the any-hit records carry the texture's extent and first quad
        k_alpha_tris<<<(r->accel.tree.slots + 255) / 256, 256, 0, r->stream>>>(r->accel.tree.slots, r->accel.tree.tris.p, r->accel.tree.shadeTris.p, makeSceneView(r), sc.alphaTexOf.p, sc.alphaTex.p, r->accel.tree.alphaTris.p);
    HIP_TRY(r, hipEventRecord(st->evCommitted, r->stream));
    HIP_TRY(r, hipGetLastError());
    st->commits++;
    if (committed)
        *committed = n;
    return PTX_OK;
}

static int textureResidency(PtxRenderer *r, uint32_t *resident, uint32_t *pending)
{
    if (!r)
        return PTX_ERROR_INVALID_ARGUMENT;
    const PtxRenderer *s = sceneOf(r);
    if (!s->link.ready)
        return fail(r, PTX_ERROR_NOT_READY, "ptx_texture_residency: no scene uploaded");
    const TextureStreaming *st = s->scene.streaming.get();
    uint32_t notResident = 0;
    if (st)
        for (uint8_t v : st->state)
            notResident += v != kTexResident;
    if (resident) *resident = s->scene.textureCount - notResident;
    if (pending) *pending = notResident;
    return PTX_OK;
}

// TextureUploader's m_RejectedCount, with the indices.
static uint32_t texturesRejected(PtxRenderer *r, uint32_t *indices, uint32_t capacity)
{
    if (!r)
        return 0;
    const PtxRenderer *s = sceneOf(r);
    if (!s->link.ready)
        return 0;
    const std::vector<uint32_t> &rej = s->scene.rejectedTextures;
    for (uint32_t k = 0; indices && k < capacity && k < rej.size(); k++)
        indices[k] = rej[k];
    return (uint32_t)rej.size();
}
