// pt_scene_host.hpp -- host side of the scene: ptx_share_scene and ptx_scene_upload.  An upload is a checked plan, then named
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
    if (owner->sceneOwner || !r->sceneSharers.empty())
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "ptx_share_scene: the owner must hold its own scene, and a renderer others share from cannot borrow");
    if (owner->device != r->device)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "ptx_share_scene: renderers on different devices (%d, %d)", r->device, owner->device);
    if (!owner->sceneReady || !owner->accelReady)
        return fail(r, PTX_ERROR_NOT_READY, "ptx_share_scene: the owner needs ptx_scene_upload and ptx_build_accel first");
    HIP_TRY(r, hipSetDevice(r->device));
    // the owner's uploads and build are enqueued on ITS stream: finished before any stream of the borrower reads them;
    // the borrower's own frames in flight end before its scene goes away
    HIP_TRY(r, hipStreamSynchronize(owner->stream));
    HIP_TRY(r, hipStreamSynchronize(r->stream));
    if (r->auxStream)
        HIP_TRY(r, hipStreamSynchronize(r->auxStream));
    detachSharedScene(r);
    // its own copies are not needed any more
    r->scene = SceneData();
    r->nodes.release(); r->tris.release(); r->shadeTris.release(); r->alphaTris.release();
    r->build = PtxRenderer::BuildState();
    r->sceneReady = false;
    r->sceneOwner = owner;
    owner->sceneSharers.push_back(r);
    r->accelReady = true;
    r->hintSlots = 0u; // whatever this handle had learnt, it had learnt on another scene
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

// TextureUploader::DetermineMaxTextureSizes (TextureUploader.cpp:551-569): the largest square extent whose full chain
// fits the per-texture share of the budget (Config.h:63-64,162-163: min(80 % of the device memory, 1 GiB)), per format;
// forceFullTextureSize keeps MaxTextureDataSize = 4096 (TextureUploader.h:74).  Block-compressed files arrive decoded
// to RGBA8 and are budgeted as that.
static void maxTextureExtents(const PtxSceneDesc *s, uint32_t textureCount, uint64_t deviceTotalBytes, uint32_t maxExtent[3])
{
    maxExtent[0] = maxExtent[1] = maxExtent[2] = 4096u;
    if (s->forceFullTextureSize || !textureCount || s->textureMemoryBudget == ~0ull)
        return;
    const uint64_t budget = s->textureMemoryBudget ? s->textureMemoryBudget : std::min<uint64_t>(deviceTotalBytes / 100u * 80u, 1024ull << 20);
    for (uint32_t f = 0; f <= PTX_TEXTURE_RGBA32F; f++)
        for (uint32_t &m = maxExtent[f]; m > 1u && chainTexels(m, m, fullLevels(m, m)) * (f == PTX_TEXTURE_RGBA32F ? 16u : 4u) > budget / textureCount;)
            m >>= 1;
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
    uint32_t maxExtent[3];
    maxTextureExtents(s, plan.textureCount, deviceTotalBytes, maxExtent);
    plan.place.resize(plan.total);
    plan.table.resize(plan.total);
    uint32_t scaled = 0;
    for (uint32_t i = 0; i < plan.total; i++)
    {
        const PtxTextureDesc &d = textureDescOf(s, plan.textureCount, i);
        DevTexture &t = plan.table[i];
        Placement &pl = plan.place[i];
        if (d.format > PTX_TEXTURE_RGBA32F)
            return fail(r, PTX_ERROR_INVALID_ARGUMENT, "texture %u: unknown format %u", i, d.format);
        pl = { d.width ? d.width : 1, d.height ? d.height : 1, d.levels ? d.levels : 1u, 0u, false, 0u, -1 };
        t = { pl.srcW, pl.srcH, 1u, d.format, {} };
        if (i < plan.textureCount)
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
    if (plan.n8 + plan.scratch8 > 0xffffffffull || plan.nf + plan.scratchF > 0xffffffffull || (uint64_t)plan.nf + plan.n8 > 0xffffffffull)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "texture pool exceeds 2^32 texels");
    plan.renderTable.assign(plan.table.begin(), plan.table.begin() + plan.total);
    for (DevTexture &t : plan.renderTable)
        if (t.format != PTX_TEXTURE_RGBA32F)
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
    return upload(r, sc.pairFirst, flat.pairFirst.data(), flat.pairFirst.size());
}

// Stage 5 (row N1): every texture into the pools of the upload formats -- the file's own chain, or its level 0 (scaled through the
// scratch chain where the plan says so) and the mip chain below it level by level on the device --, then decoded into the pool the
// render kernels sample.  The upload-format pools are this stage's own: freed when it returns, whichever way (hipFree waits).
static int uploadTextures(PtxRenderer *r, const PtxSceneDesc *s, const TexturePlan &plan)
{
    SceneData &sc = r->scene;
    DevBuf<DevTexture> textures; // upload time only: the table, the pools of the image formats in which mip chains are built,
    DevBuf<uint32_t> texels8;    // the sRGB byte -> linear table
    DevBuf<float4> texelsF;
    DevBuf<float> srgbLut;
    HIP_TRY(r, srgbLut.alloc(256));
    k_build_srgb_lut<<<1, 256, 0, r->stream>>>(srgbLut.p);
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
        else if (d.data)
            HIP_TRY(r, hipMemcpyAsync(poolAt(t.levelOffset[0]), d.data, (size_t)t.width * t.height * texel, hipMemcpyHostToDevice, r->stream));
        for (uint32_t l = 1; l < t.levels; l++)
            blit(i, l - 1, i, l);
    }
    // The pool the render kernels sample (pt_device.hpp, fetchTexel): every level of every texture decoded to four floats,
    // the RGBA32F pool first, the 8-bit textures behind it; `renderTextures` is the table with offsets into that pool.
    HIP_TRY(r, sc.renderTexels.alloc(plan.nf + plan.n8));
    HIP_TRY(r, sc.renderTextures.alloc(plan.total));
    if (plan.nf)
        HIP_TRY(r, hipMemcpyAsync(sc.renderTexels.p, texelsF.p, plan.nf * sizeof(float4), hipMemcpyDeviceToDevice, r->stream));
    for (uint32_t i = 0; i < plan.total; i++)
    {
        const DevTexture &t = plan.table[i];
        if (t.format == PTX_TEXTURE_RGBA32F)
            continue;
        const size_t count = chainTexels(t.width, t.height, t.levels);
        const uint32_t first = t.levelOffset[0];
        k_decode_texels<<<(uint32_t)((count + 255) / 256), 256, 0, r->stream>>>(texels8.p, srgbLut.p, first, (uint32_t)count, t.format,
                                                                              sc.renderTexels.p + plan.nf + first);
    }
    if (plan.total)
        HIP_TRY(r, hipMemcpyAsync(sc.renderTextures.p, plan.renderTable.data(), plan.total * sizeof(DevTexture), hipMemcpyHostToDevice, r->stream));
    HIP_TRY(r, hipStreamSynchronize(r->stream)); // the caller's texel arrays may go away, and the pools of the upload formats do
    HIP_TRY(r, hipGetLastError());
    return PTX_OK;
}

// Stage 6: what the any-hit stages read of the textures.
static int alphaFootprints(PtxRenderer *r, const TexturePlan &plan)
{
    SceneData &sc = r->scene;
    int rc;
    if (sc.anyNonOpaque)
        HIP_TRY(r, sc.alphaQuads.alloc(plan.alphaQuads));
    for (uint32_t ti = 0; ti < plan.textureCount; ti++)
        if (plan.alphaTexOf[ti] != kNoAlphaTex)
        {
            const AlphaTex &at = plan.alphaTex[plan.alphaTexOf[ti]];
            k_alpha_quads<<<(at.width * at.height + 255) / 256, 256, 0, r->stream>>>(at.width, at.height, sc.renderTexels.p + plan.renderTable[ti].levelOffset[0],
                                                                                    sc.alphaQuads.p + at.offset);
        }
    if ((rc = upload(r, sc.alphaTex, plan.alphaTex.data(), plan.alphaTex.size())) != PTX_OK) return rc;
    return upload(r, sc.alphaTexOf, plan.alphaTexOf.data(), plan.alphaTexOf.size());
}

static int sceneUpload(PtxRenderer *r, const PtxSceneDesc *s)
{
    if (!r || !s)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "ptx_scene_upload: null argument");
    HIP_TRY(r, hipSetDevice(r->device));
    // The plan: host only.  A description that is refused here leaves the handle as it was -- its own scene, or the one it
    // borrows -- and nothing below refuses one.
    int rc;
    FlatScene flat;
    TexturePlan plan;
    size_t freeB = 0, totalB = 0;
    if ((rc = validateSceneDesc(r, s)) != PTX_OK) return rc;
    if ((rc = flattenScene(r, s, flat)) != PTX_OK) return rc;
    if (!s->forceFullTextureSize && s->textures && s->textureCount && !s->textureMemoryBudget) // the one case planTextures reads it in
        HIP_TRY(r, hipMemGetInfo(&freeB, &totalB));
    if ((rc = planTextures(r, s, totalB, flat.anyNonOpaque, plan)) != PTX_OK) return rc;

    // from here on the old scene is gone, whatever happens
    detachSharedScene(r); // a renderer that was borrowing a scene gets its own again
    quiesceSharers(r);
    r->sceneReady = r->accelReady = false;
    r->sceneEpoch++;
    r->build = PtxRenderer::BuildState();
    if ((rc = uploadGeometry(r, s, flat)) != PTX_OK) return rc;
    if ((rc = uploadTextures(r, s, plan)) != PTX_OK) return rc;
    if ((rc = alphaFootprints(r, plan)) != PTX_OK) return rc;
    HIP_TRY(r, hipStreamSynchronize(r->stream)); // `flat`, `plan` and the caller's arrays may go away
    r->sceneReady = true;
    r->stats.triangles = flat.triangles;
    return PTX_OK;
}
