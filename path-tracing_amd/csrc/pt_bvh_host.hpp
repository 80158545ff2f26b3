// pt_bvh_host.hpp -- host side of the tree build (kernels: pt_bvh_build.hpp): the scan and sort helpers, the level lists, the
// stages of one build, buildAccel that strings them together, and buildBestTree that prices a few trees and keeps the cheapest.
// Included by pt_runtime.hpp below the renderer object (PtxRenderer, DevBuf, HIP_TRY, fail); a stage returns a PTX_* code.  The state
// is AccelState, the member `accel` of the handle: the Tree in use (its four buffers and the three numbers that describe them move
// together), the BuildState a refit reuses, the TreeParams.
#pragma once

// Exclusive scan in place of `count` 32-bit counts; blockSums holds one word per kScan32Block counts (unused for one block).
static void scanExclusive32(hipStream_t stream, uint32_t count, uint32_t *data, uint32_t *blockSums)
{
    const uint32_t blocks = (count + kScan32Block - 1) / kScan32Block;
    if (blocks > 1)
    {
        k_scan32_sums<<<blocks, 256, 0, stream>>>(count, data, blockSums);
        k_scan_exclusive<<<1, 1024, 0, stream>>>(blocks, blockSums);
        k_scan32_apply<<<blocks, 256, 0, stream>>>(count, data, blockSums);
    }
    else
        k_scan_exclusive<<<1, 1024, 0, stream>>>(count, data);
}

// One 8-bit pass of the LSD radix sort of pt_bvh_build.hpp over `count` (key, value) pairs; hist / histSums sized by the caller.
static void radixPass(PtxRenderer *r, uint32_t count, const uint64_t *kin, const uint32_t *vin, uint64_t *kout, uint32_t *vout, uint32_t shift,
                      uint32_t *hist, uint32_t *histSums)
{
    const uint32_t numTiles = (count + kSortTile - 1) / kSortTile;
    k_sort_hist<<<numTiles, 64, 0, r->stream>>>(count, kin, shift, numTiles, hist);
    scanExclusive32(r->stream, 256 * numTiles, hist, histSums);
    k_sort_scatter<<<numTiles, 64, 0, r->stream>>>(count, kin, vin, kout, vout, shift, numTiles, hist);
}

// The leaf references of one build, which everything from the Morton sort on works over: one per triangle (the triangles' own
// boxes; tri == nullptr is the identity), the pieces of split triangles, or pairs of triangles (pair != nullptr).
struct RefSet
{
    uint32_t n = 0;                          // references, the zero-area ones included
    const float4 *lo = nullptr, *hi = nullptr; // box per reference
    const uint8_t *inert = nullptr;          // per reference: left out of the tree (zero area)
    const uint32_t *tri = nullptr;           // reference -> (first) triangle
    const uint8_t *pair = nullptr;           // per reference: the next triangle is in it too
};

// Level lists of the CURRENT binary topology over nv leaves (B.children / B.parentOfNode): B.levelOrder, B.levelStart.
// B.levelsValid stays false: the tree is deeper than kMaxTreeLevels (or is not a tree) and the caller takes the fence-and-atomic
// kernels.  Scratch: B.keys0 / keys1 (the Morton keys are done with), B.hist / histSums.
static int treeLevels(PtxRenderer *r, uint32_t nv)
{
    BuildState &B = r->accel.build;
    B.levelsValid = false;
    if (nv < 2)
        return PTX_OK;
    const uint32_t nodes = nv - 1, blocks = (nodes + 255) / 256;
    HIP_TRY(r, B.lvDepth0.alloc(nodes)); HIP_TRY(r, B.lvDepth1.alloc(nodes)); HIP_TRY(r, B.lvAnc0.alloc(nodes)); HIP_TRY(r, B.lvAnc1.alloc(nodes));
    HIP_TRY(r, B.lvVals0.alloc(nodes)); HIP_TRY(r, B.lvVals1.alloc(nodes)); HIP_TRY(r, B.lvStartDev.alloc(kMaxTreeLevels + 2));
    uint32_t *d0 = B.lvDepth0.p, *d1 = B.lvDepth1.p, *flag = B.lvStartDev.p; // (flag: the first word, before the starts are written)
    int *a0 = B.lvAnc0.p, *a1 = B.lvAnc1.p;
    k_depth_init<<<blocks, 256, 0, r->stream>>>((int)nodes, B.parentOfNode.p, d0, a0);
    bool done = false;
    for (uint32_t pass = 0; pass < 24 && !done; pass++) // pass k covers paths of 2^(k + 1) links
    {
        HIP_TRY(r, hipMemsetAsync(flag, 0, sizeof(uint32_t), r->stream));
        k_depth_jump<<<blocks, 256, 0, r->stream>>>((int)nodes, d0, a0, d1, a1, flag);
        std::swap(d0, d1);
        std::swap(a0, a1);
        if (pass >= 4) // (a tree of 64 or more leaves is at least six deep: no point in asking earlier)
        {
            uint32_t pending = 0;
            HIP_TRY(r, hipMemcpyAsync(&pending, flag, sizeof(pending), hipMemcpyDeviceToHost, r->stream));
            HIP_TRY(r, hipStreamSynchronize(r->stream));
            done = pending == 0;
        }
    }
    if (!done)
        return PTX_OK; // a parent chain longer than 2^24: not a tree the level passes can take
    uint32_t maxDepth = 0;
    HIP_TRY(r, hipMemsetAsync(flag, 0, sizeof(uint32_t), r->stream));
    k_depth_keys<<<blocks, 256, 0, r->stream>>>((int)nodes, d0, B.keys0.p, B.lvVals0.p, flag);
    HIP_TRY(r, hipMemcpyAsync(&maxDepth, flag, sizeof(maxDepth), hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(r, hipStreamSynchronize(r->stream));
    if (maxDepth >= kMaxTreeLevels)
        return PTX_OK;
    const uint64_t *sortedKeys = B.keys1.p;
    radixPass(r, nodes, B.keys0.p, B.lvVals0.p, B.keys1.p, B.lvVals1.p, 0, B.hist.p, B.histSums.p);
    B.levelOrder = B.lvVals1.p;
    if (maxDepth > 255)
    {
        radixPass(r, nodes, B.keys1.p, B.lvVals1.p, B.keys0.p, B.lvVals0.p, 8, B.hist.p, B.histSums.p);
        B.levelOrder = B.lvVals0.p;
        sortedKeys = B.keys0.p;
    }
    k_level_starts<<<blocks, 256, 0, r->stream>>>((int)nodes, sortedKeys, B.lvStartDev.p);
    B.levelStart.assign(maxDepth + 2, 0u);
    HIP_TRY(r, hipMemcpyAsync(B.levelStart.data(), B.lvStartDev.p, (maxDepth + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(r, hipStreamSynchronize(r->stream));
    B.levelStart[maxDepth + 1] = nodes;
    for (uint32_t d = 0; d <= maxDepth; d++) // every depth up to the deepest holds a node, in order
        if (B.levelStart[d] >= B.levelStart[d + 1])
            return PTX_OK;
    B.levelsValid = true;
    return PTX_OK;
}

// One bottom-up pass over the current binary topology of the nv sorted references: the node boxes, or (price) T(x, 1..4) and
// the collapse decision per node.  Over the level lists, one launch per level, deepest first -- asked for here if the caller
// says so (the topology changed; a refit has them from the last full build); the fence-and-atomic climb, after clearing its
// arrival flags, only for a tree the lists cannot take or with PTX_FENCE_REFIT.
static int bottomUpPass(PtxRenderer *r, const RefSet &refs, uint32_t nv, bool price, bool askForLists)
{
    BuildState &B = r->accel.build;
    int rc;
    if (askForLists && !r->env.fenceRefit && (rc = treeLevels(r, nv)) != PTX_OK)
        return rc;
    if (B.levelsValid && !r->env.fenceRefit)
        for (size_t d = B.levelStart.size() - 1; d-- > 0;)
        {
            const uint32_t first = B.levelStart[d], count = B.levelStart[d + 1] - first, blocks = (count + 255) / 256;
            if (price)
                k_collapse_cost_level<<<blocks, 256, 0, r->stream>>>(first, count, B.levelOrder, B.vals0.p, refs.lo, refs.hi, B.children.p, B.nodeLo.p, B.nodeHi.p,
                                                                    B.collapseCost.p, B.collapseDecide.p);
            else
                k_refit_level<<<blocks, 256, 0, r->stream>>>(first, count, B.levelOrder, B.vals0.p, refs.lo, refs.hi, B.children.p, B.nodeLo.p, B.nodeHi.p);
        }
    else
    {
        HIP_TRY(r, hipMemsetAsync(B.flags.p, 0, (size_t)nv * 4, r->stream));
        if (price)
            k_collapse_cost<<<(nv + 255) / 256, 256, 0, r->stream>>>((int)nv, B.vals0.p, refs.lo, refs.hi, B.children.p, B.parentOfNode.p, B.parentOfLeaf.p, B.nodeLo.p,
                                                                    B.nodeHi.p, B.flags.p, B.collapseCost.p, B.collapseDecide.p);
        else
            k_refit<<<(nv + 255) / 256, 256, 0, r->stream>>>((int)nv, B.vals0.p, refs.lo, refs.hi, B.children.p, B.parentOfNode.p, B.parentOfLeaf.p, B.nodeLo.p,
                                                            B.nodeHi.p, B.flags.p);
    }
    return PTX_OK;
}

// Per triangle: world-space record, padded box, zero-area flag; the build's timed span starts here.  A full build starts from
// no tree: it invalidates the kept state (the buffers stay for reuse).
static int triangleRecords(PtxRenderer *r, bool refit)
{
    BuildState &B = r->accel.build;
    const uint32_t nTri = r->scene.triCount;
    if (!refit)
    {
        B.valid = false;
        // the level lists describe the topology of the LAST build: a full build starts without them (a build whose reinsertion
        // passes do not run -- PTX_REINSERT=0, a broken pass, the rebuild after a revived triangle -- would otherwise price its
        // collapse in the order and over the node count of an older tree)
        B.levelsValid = false;
        B.levelOrder = nullptr;
        B.levelStart.clear();
        HIP_TRY(r, B.triTmp.alloc(nTri)); HIP_TRY(r, B.boxLo.alloc(nTri)); HIP_TRY(r, B.boxHi.alloc(nTri)); HIP_TRY(r, B.inert.alloc(nTri));
        HIP_TRY(r, B.sceneBounds.alloc(8));
    }
    // [0..5] centroid bounds (ordered floats), [6] references in the tree (k_count_valid), [7] a refit found a revived triangle
    const uint32_t initBounds[8] = { 0xffffffffu, 0xffffffffu, 0xffffffffu, 0u, 0u, 0u, 0u, 0u };
    HIP_TRY(r, hipMemcpyAsync(B.sceneBounds.p, initBounds, sizeof(initBounds), hipMemcpyHostToDevice, r->stream));
    HIP_TRY(r, hipEventRecord(r->launch.evA.get(), r->stream));
    k_tri_setup<<<(nTri + 255) / 256, 256, 0, r->stream>>>(nTri, r->scene.pairCount, r->scene.pairFirst.p, r->scene.pairs.p, r->scene.vertices.p, r->scene.indices.p, B.triTmp.p,
                                                          B.boxLo.p, B.boxHi.p, B.sceneBounds.p, B.inert.p, refit ? 1 : 0);
    return PTX_OK;
}

// References by splitting: the pieces of the triangles worth it into B.refLo / refHi / refTri / refInert.  *n is the number
// of references made; left alone if the budget buys none.
static int splitReferences(PtxRenderer *r, uint32_t *n)
{
    BuildState &B = r->accel.build;
    const uint32_t nTri = r->scene.triCount, tb = (nTri + 255) / 256;
    DevBuf<float> priority;
    DevBuf<uint32_t> count, sums;
    DevBuf<unsigned long long> sum;
    HIP_TRY(r, priority.alloc(nTri)); HIP_TRY(r, count.alloc((size_t)nTri + 1)); HIP_TRY(r, sums.alloc((nTri + 1 + kScan32Block - 1) / kScan32Block));
    HIP_TRY(r, sum.alloc(1)); HIP_TRY(r, hipMemsetAsync(sum.p, 0, sizeof(unsigned long long), r->stream));
    k_split_priority<<<tb, 256, 0, r->stream>>>(nTri, B.triTmp.p, B.boxLo.p, B.boxHi.p, B.inert.p, B.sceneBounds.p, r->accel.params.mortonCubic ? 1 : 0, priority.p, sum.p);
    unsigned long long total = 0;
    HIP_TRY(r, hipMemcpyAsync(&total, sum.p, sizeof(total), hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(r, hipStreamSynchronize(r->stream));
    if (!total)
        return PTX_OK;
    const float perPriority = (float)((double)r->accel.params.splitBudget * nTri / ((double)total / kSplitPriorityScale));
    HIP_TRY(r, hipMemsetAsync(count.p + nTri, 0, sizeof(uint32_t), r->stream));
    k_split_count<<<tb, 256, 0, r->stream>>>(nTri, priority.p, perPriority, count.p);
    scanExclusive32(r->stream, nTri + 1, count.p, sums.p);
    uint32_t refs = 0;
    HIP_TRY(r, hipMemcpyAsync(&refs, count.p + nTri, sizeof(refs), hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(r, hipStreamSynchronize(r->stream));
    if (refs <= nTri || refs > kMaxTriangles)
        return PTX_OK;
    HIP_TRY(r, B.refLo.alloc(refs)); HIP_TRY(r, B.refHi.alloc(refs)); HIP_TRY(r, B.refTri.alloc(refs)); HIP_TRY(r, B.refInert.alloc(refs));
    k_split_write<<<tb, 256, 0, r->stream>>>(nTri, B.triTmp.p, B.boxLo.p, B.boxHi.p, B.inert.p, B.sceneBounds.p, r->accel.params.mortonCubic ? 1 : 0, count.p, refs,
                                            B.refLo.p, B.refHi.p, B.refTri.p, B.refInert.p);
    HIP_TRY(r, hipStreamSynchronize(r->stream)); // (count and priority go out of scope)
    *n = refs;
    return PTX_OK;
}

// References by pairing (pt_bvh_build.hpp, "pair leaves"): B.refTri / refPair / refInert; their boxes are k_ref_boxes's to
// write.  *n is the number of references made; left alone if no two triangles pair.
static int pairReferences(PtxRenderer *r, uint32_t *n)
{
    BuildState &B = r->accel.build;
    const uint32_t nTri = r->scene.triCount, tb = (nTri + 255) / 256;
    DevBuf<uint8_t> link;
    DevBuf<uint32_t> s0, s1, head, sums;
    HIP_TRY(r, link.alloc(nTri)); HIP_TRY(r, s0.alloc(nTri)); HIP_TRY(r, s1.alloc(nTri)); HIP_TRY(r, head.alloc((size_t)nTri + 1));
    HIP_TRY(r, sums.alloc((nTri + 1 + kScan32Block - 1) / kScan32Block));
    k_pair_links<<<tb, 256, 0, r->stream>>>(nTri, B.triTmp.p, r->scene.pairs.p, r->scene.indices.p, B.boxLo.p, B.boxHi.p, B.inert.p, link.p);
    k_pair_jump<<<tb, 256, 0, r->stream>>>(nTri, link.p, nullptr, s0.p);
    for (uint32_t span = 1; span < nTri; span *= 2) // after k jumps a run start up to 2^k positions back is found
    {
        k_pair_jump<<<tb, 256, 0, r->stream>>>(nTri, link.p, s0.p, s1.p);
        s0.swap(s1);
    }
    HIP_TRY(r, hipMemsetAsync(head.p + nTri, 0, sizeof(uint32_t), r->stream));
    k_pair_heads<<<tb, 256, 0, r->stream>>>(nTri, link.p, s0.p, head.p);
    scanExclusive32(r->stream, nTri + 1, head.p, sums.p);
    uint32_t refs = 0;
    HIP_TRY(r, hipMemcpyAsync(&refs, head.p + nTri, sizeof(refs), hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(r, hipStreamSynchronize(r->stream));
    if (refs >= nTri)
        return PTX_OK;
    HIP_TRY(r, B.refLo.alloc(refs)); HIP_TRY(r, B.refHi.alloc(refs)); HIP_TRY(r, B.refTri.alloc(refs)); HIP_TRY(r, B.refInert.alloc(refs));
    HIP_TRY(r, B.refPair.alloc(refs)); HIP_TRY(r, B.slotOf.alloc((size_t)refs + 1));
    k_pair_write<<<tb, 256, 0, r->stream>>>(nTri, link.p, s0.p, head.p, B.inert.p, B.refTri.p, B.refPair.p, B.refInert.p);
    HIP_TRY(r, hipStreamSynchronize(r->stream)); // (the temporaries go out of scope)
    *n = refs;
    return PTX_OK;
}

// The reference set of this build.  A full build makes it: one reference per triangle, or the pieces of the triangles worth
// splitting (static scenes: a build that keeps its state for refits does not split), or pair leaves (not with pre-splitting).
// A refit keeps the references of the last full build, and recomputes the union boxes of the pairs like a full build does.
static int leafReferences(PtxRenderer *r, bool refit, bool keepState, RefSet *refs)
{
    BuildState &B = r->accel.build;
    const uint32_t nTri = r->scene.triCount;
    uint32_t n = refit ? B.refCount : nTri;
    int rc;
    if (!refit)
    {
        if (!keepState && r->accel.params.splitBudget > 0.0f && nTri > 1 && (rc = splitReferences(r, &n)) != PTX_OK)
            return rc;
        if (r->env.pairLeaves && r->accel.params.splitBudget <= 0.0f && nTri > 1 && (rc = pairReferences(r, &n)) != PTX_OK)
            return rc;
        B.pairRefs = n < nTri;
        B.refCount = n;
    }
    if (B.pairRefs)
        k_ref_boxes<<<(n + 255) / 256, 256, 0, r->stream>>>(n, B.refTri.p, B.refPair.p, B.boxLo.p, B.boxHi.p, B.refLo.p, B.refHi.p);
    if (n == nTri) // (splitting makes more references than triangles, pairing fewer)
        *refs = { n, B.boxLo.p, B.boxHi.p, B.inert.p, nullptr, nullptr };
    else
        *refs = { n, B.refLo.p, B.refHi.p, B.refInert.p, B.refTri.p, B.pairRefs ? B.refPair.p : nullptr };
    return PTX_OK;
}

// PLOC temporaries: two cluster sequences, neighbour indices, scan flags (sized for all n; freed when the build returns)
struct PlocScratch
{
    DevBuf<int> cl0, cl1;
    DevBuf<float4> lo0, hi0, lo1, hi1;
    DevBuf<uint32_t> nn;
    DevBuf<unsigned long long> flags, sums, total;
};

// What a full build needs per reference, the tree's own arrays included (a refit reuses all of it).
static int referenceBuffers(PtxRenderer *r, uint32_t n, uint32_t slotCap, PlocScratch &ploc)
{
    BuildState &B = r->accel.build;
    const uint32_t histCount = 256 * ((n + kSortTile - 1) / kSortTile);
    HIP_TRY(r, r->accel.tree.nodes.alloc(n)); // (as many as the emitted array: the two change places in the depth-first relayout)
    HIP_TRY(r, r->accel.tree.tris.alloc(slotCap)); HIP_TRY(r, r->accel.tree.shadeTris.alloc(slotCap));
    HIP_TRY(r, B.nodeLo.alloc(n)); HIP_TRY(r, B.nodeHi.alloc(n)); HIP_TRY(r, B.vals0.alloc(n)); HIP_TRY(r, B.vals1.alloc(n));
    HIP_TRY(r, B.hist.alloc(histCount)); HIP_TRY(r, B.histSums.alloc((histCount + kScan32Block - 1) / kScan32Block)); HIP_TRY(r, B.flags.alloc(n));
    HIP_TRY(r, B.keys0.alloc(n)); HIP_TRY(r, B.keys1.alloc(n));
    HIP_TRY(r, B.children.alloc(n)); HIP_TRY(r, B.parentOfNode.alloc(n)); HIP_TRY(r, B.parentOfLeaf.alloc(n));
    HIP_TRY(r, B.rawNodes.alloc(n)); HIP_TRY(r, B.oldOf.alloc((size_t)n + 1)); HIP_TRY(r, B.collapseCost.alloc(n)); HIP_TRY(r, B.collapseDecide.alloc(n));
    if (r->accel.usePloc && n > 1)
    {
        HIP_TRY(r, ploc.cl0.alloc(n)); HIP_TRY(r, ploc.cl1.alloc(n)); HIP_TRY(r, ploc.lo0.alloc(n)); HIP_TRY(r, ploc.hi0.alloc(n)); HIP_TRY(r, ploc.lo1.alloc(n));
        HIP_TRY(r, ploc.hi1.alloc(n)); HIP_TRY(r, ploc.nn.alloc(n)); HIP_TRY(r, ploc.flags.alloc(n)); HIP_TRY(r, ploc.sums.alloc((n + kScanBlock - 1) / kScanBlock));
        HIP_TRY(r, ploc.total.alloc(1));
    }
    return PTX_OK;
}

// Morton sort of the references: the sorted order in B.keys0 / B.vals0, B.treeTris = the references in the tree (all but the
// zero-area ones, which sort to the end), B.slotOf for pair leaves.  Kept for refits.
static int sortReferences(PtxRenderer *r, const RefSet &refs)
{
    BuildState &B = r->accel.build;
    k_morton<<<(refs.n + 255) / 256, 256, 0, r->stream>>>(refs.n, refs.lo, refs.hi, B.sceneBounds.p, refs.inert, B.keys0.p, B.vals0.p, r->accel.params.mortonCubic ? 1 : 0);
    // 63-bit keys + the all-ones sentinel of inert triangles: 8 passes, which ping-pong the buffers an even number of times
    for (uint32_t shift = 0; shift < 64; shift += 16)
    {
        radixPass(r, refs.n, B.keys0.p, B.vals0.p, B.keys1.p, B.vals1.p, shift, B.hist.p, B.histSums.p);
        radixPass(r, refs.n, B.keys1.p, B.vals1.p, B.keys0.p, B.vals0.p, shift + 8, B.hist.p, B.histSums.p);
    }
    k_count_valid<<<1, 1, 0, r->stream>>>(refs.n, B.keys0.p, &B.sceneBounds.p[6]);
    uint32_t nv = 0;
    HIP_TRY(r, hipMemcpyAsync(&nv, &B.sceneBounds.p[6], sizeof(nv), hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(r, hipStreamSynchronize(r->stream));
    B.treeTris = nv;
    if (B.pairRefs) // the first triangle slot of every sorted reference (kept for refits, whose order is the same)
    {
        DevBuf<uint32_t> sums;
        HIP_TRY(r, sums.alloc((nv + 1 + kScan32Block - 1) / kScan32Block));
        k_slot_sizes<<<(nv + 1 + 255) / 256, 256, 0, r->stream>>>(nv, B.vals0.p, B.refPair.p, B.slotOf.p);
        scanExclusive32(r->stream, nv + 1, B.slotOf.p, sums.p);
        HIP_TRY(r, hipStreamSynchronize(r->stream)); // (sums goes out of scope)
    }
    return PTX_OK;
}

// Binary topology over the nv sorted references, with its boxes: PLOC (which computes them as it merges), or Karras.
static int binaryTopology(PtxRenderer *r, const RefSet &refs, uint32_t nv, PlocScratch &ploc)
{
    BuildState &B = r->accel.build;
    if (!r->accel.usePloc)
    {
        k_karras<<<(nv + 255) / 256, 256, 0, r->stream>>>((int)nv, B.keys0.p, B.children.p, B.parentOfNode.p, B.parentOfLeaf.p);
        return bottomUpPass(r, refs, nv, false, true);
    }
    k_ploc_init<<<(nv + 255) / 256, 256, 0, r->stream>>>(nv, B.vals0.p, refs.lo, refs.hi, ploc.cl0.p, ploc.lo0.p, ploc.hi0.p);
    int *cIn = ploc.cl0.p, *cOut = ploc.cl1.p;
    float4 *lIn = ploc.lo0.p, *hIn = ploc.hi0.p, *lOut = ploc.lo1.p, *hOut = ploc.hi1.p;
    uint32_t count = nv;
    int nextId = (int)nv - 2;
    uint32_t iterations = 0;
    while (count > 1)
    {
        const uint32_t cb = (count + 255) / 256, sb = (count + kScanBlock - 1) / kScanBlock;
        k_ploc_nearest<<<cb, 256, 0, r->stream>>>(count, r->accel.params.plocRadius, r->accel.params.plocShape, lIn, hIn, ploc.nn.p);
        k_ploc_flags<<<cb, 256, 0, r->stream>>>(count, ploc.nn.p, ploc.flags.p);
        k_scan64_sums<<<sb, 256, 0, r->stream>>>(count, ploc.flags.p, ploc.sums.p);
        k_scan64_top<<<1, 1024, 0, r->stream>>>(sb, ploc.sums.p, ploc.total.p);
        k_scan64_apply<<<sb, 256, 0, r->stream>>>(count, ploc.flags.p, ploc.sums.p);
        k_ploc_merge<<<cb, 256, 0, r->stream>>>(count, cIn, lIn, hIn, ploc.nn.p, ploc.flags.p, nextId, cOut, lOut, hOut, B.children.p, B.parentOfNode.p,
                                                B.parentOfLeaf.p, B.nodeLo.p, B.nodeHi.p);
        unsigned long long t = 0;
        HIP_TRY(r, hipMemcpyAsync(&t, ploc.total.p, sizeof(t), hipMemcpyDeviceToHost, r->stream));
        HIP_TRY(r, hipStreamSynchronize(r->stream));
        const uint32_t kept = (uint32_t)t, merged = (uint32_t)(t >> 32);
        if (merged == 0 || kept + merged != count)
            return fail(r, PTX_ERROR_DEVICE, "ptx_build_accel: PLOC made no progress (%u clusters, %u kept, %u merged)", count, kept, merged);
        nextId -= (int)merged;
        count = kept;
        std::swap(cIn, cOut);
        std::swap(lIn, lOut);
        std::swap(hIn, hOut);
        iterations++;
    }
    if (r->env.verbose)
        std::fprintf(stderr, "[ptx] PLOC: %u triangles (%u inert left out), %u iterations\n", nv, refs.n - nv, iterations);
    return PTX_OK;
}

// `passes` of parallel reinsertion over the binary tree (k_reinsert_find / _claim / _apply), boxes recomputed after every pass.
// *broken: a pass left something that is not a tree; the caller starts the build again (this handle reinserts no more).
static int reinsertionPasses(PtxRenderer *r, const RefSet &refs, uint32_t nv, uint32_t passes, bool *broken)
{
    BuildState &B = r->accel.build;
    const uint32_t slots = 2 * nv - 1, sblocks = (slots + 255) / 256;
    DevBuf<int> target, top;
    DevBuf<float> gain;
    DevBuf<unsigned long long> lock;
    DevBuf<uint32_t> applied, counts;
    HIP_TRY(r, target.alloc(slots)); HIP_TRY(r, top.alloc(slots)); HIP_TRY(r, gain.alloc(slots)); HIP_TRY(r, lock.alloc(slots)); HIP_TRY(r, applied.alloc(1));
    HIP_TRY(r, counts.alloc(3));
    int rc;
    const ReinsertTree rt = { (int)nv, B.children.p, B.parentOfNode.p, B.parentOfLeaf.p, B.nodeLo.p, B.nodeHi.p, B.vals0.p, refs.lo, refs.hi };
    for (uint32_t pass = 0; pass < passes; pass++)
    {
        HIP_TRY(r, hipMemsetAsync(lock.p, 0, (size_t)slots * sizeof(unsigned long long), r->stream));
        HIP_TRY(r, hipMemsetAsync(applied.p, 0, sizeof(uint32_t), r->stream));
        k_reinsert_find<<<sblocks, 256, 0, r->stream>>>(rt, 1u, 0u, target.p, gain.p, top.p);
        k_reinsert_claim<<<sblocks, 256, 0, r->stream>>>(rt, target.p, gain.p, top.p, lock.p);
        k_reinsert_apply<<<sblocks, 256, 0, r->stream>>>(rt, target.p, gain.p, top.p, lock.p, applied.p);
        // still a tree?  (a knot would hang k_refit: checked BEFORE the boxes are recomputed)
        uint32_t moved = 0, check[3] = { 0, 0, 0 };
        HIP_TRY(r, hipMemsetAsync(counts.p, 0, 3 * sizeof(uint32_t), r->stream));
        k_tree_check<<<(nv + 255) / 256, 256, 0, r->stream>>>(rt, counts.p);
        HIP_TRY(r, hipMemcpyAsync(check, counts.p, sizeof(check), hipMemcpyDeviceToHost, r->stream));
        HIP_TRY(r, hipMemcpyAsync(&moved, applied.p, sizeof(moved), hipMemcpyDeviceToHost, r->stream));
        HIP_TRY(r, hipStreamSynchronize(r->stream));
        if (r->env.verbose)
            std::fprintf(stderr, "[ptx] reinsertion pass %u: %u moves; check: %u bad parent links, %u leaves off the root, longest path %u\n", pass,
                         moved, check[0], check[1], check[2]);
        if (check[0] || check[1])
        {
            // Not a tree any more (never seen since the path locks were completed, but the moves of a pass race by design):
            // this handle builds without reinsertion from now on, starting with this tree again.
            r->accel.reinsertBroken = true;
            fail(r, PTX_OK, "ptx_build_accel: reinsertion pass %u left %u bad parent links, %u leaves off the root: rebuilt without reinsertion",
                 pass, check[0], check[1]);
            if (r->env.verbose)
                std::fprintf(stderr, "[ptx] %s\n", r->error.c_str());
            *broken = true;
            break;
        }
        if ((rc = bottomUpPass(r, refs, nv, false, true)) != PTX_OK) // the pass changed the topology
            return rc;
    }
    HIP_TRY(r, hipStreamSynchronize(r->stream)); // (the pass's buffers go out of scope)
    return PTX_OK;
}

// Breadth-first relayout of the emitted nodes into the compact array (k_relayout_level: the host reads the level's end after
// each launch), then depth-first order if the tree asks for it.  stats.bvhNodes = the nodes that are live.
static int relayoutNodes(PtxRenderer *r, uint32_t n, uint32_t nv)
{
    BuildState &B = r->accel.build;
    uint32_t *nextFree = B.oldOf.p + n;
    const uint32_t first[1] = { 0u }, one = 1u;
    HIP_TRY(r, hipMemcpyAsync(B.oldOf.p, first, sizeof(first), hipMemcpyHostToDevice, r->stream)); // the root stays node 0
    HIP_TRY(r, hipMemcpyAsync(nextFree, &one, sizeof(one), hipMemcpyHostToDevice, r->stream));
    uint32_t lo = 0, hi = 1, levels = 0;
    std::vector<uint32_t> levelStart; // of the breadth-first array, plus its end
    while (lo < hi)
    {
        levelStart.push_back(lo);
        k_relayout_level<<<(hi - lo + 255) / 256, 256, 0, r->stream>>>(lo, hi, B.rawNodes.p, B.oldOf.p, nextFree, r->accel.tree.nodes.p);
        uint32_t end = 0;
        HIP_TRY(r, hipMemcpyAsync(&end, nextFree, sizeof(end), hipMemcpyDeviceToHost, r->stream));
        HIP_TRY(r, hipStreamSynchronize(r->stream));
        if (end < hi || end > nv - 1)
            return fail(r, PTX_ERROR_DEVICE, "ptx_build_accel: relayout placed %u nodes of at most %u", end, nv - 1);
        lo = hi;
        hi = end;
        levels++;
    }
    r->stats.bvhNodes = r->accel.tree.nodeCount = hi;
    if (r->accel.params.layout == 1 && hi > 1)
    {
        // depth-first order (k_subtree_size / _pos / k_place_nodes); scratch: the build's flags and the sort's second value array are done with
        levelStart.push_back(hi);
        uint32_t *size = B.flags.p, *pos = B.vals1.p;
        for (uint32_t l = levels; l-- > 0;)
            k_subtree_size<<<(levelStart[l + 1] - levelStart[l] + 255) / 256, 256, 0, r->stream>>>(levelStart[l], levelStart[l + 1], r->accel.tree.nodes.p, size);
        for (uint32_t l = 0; l < levels; l++)
            k_subtree_pos<<<(levelStart[l + 1] - levelStart[l] + 255) / 256, 256, 0, r->stream>>>(levelStart[l], levelStart[l + 1], r->accel.tree.nodes.p, size, pos);
        k_place_nodes<<<(hi + 255) / 256, 256, 0, r->stream>>>(hi, r->accel.tree.nodes.p, pos, B.rawNodes.p);
        r->accel.tree.nodes.swap(B.rawNodes); // the emitted nodes are not needed again before the next k_emit, which rewrites them all
    }
    if (r->env.verbose)
        std::fprintf(stderr, "[ptx] relayout: %u of %u emitted nodes are live, %u levels\n", hi, nv - 1, levels);
    return PTX_OK;
}

// One attempt at the tree.  A full build: triangle records, references, sort, topology with boxes, reinsertion, collapse
// pricing, emit, relayout, alpha records.  A refit: new records and reference boxes, then boxes, pricing, emit, relayout and
// alpha records over the KEPT Morton order and binary topology.  *startOver: the attempt ended without a tree and the caller
// builds in full instead -- reinsertion left something that is not a tree, or a refit found a revived triangle.
static int buildOnce(PtxRenderer *r, bool refit, bool keepState, bool *startOver)
{
    BuildState &B = r->accel.build;
    const uint32_t nTri = r->scene.triCount;
    int rc;
    RefSet refs;
    PlocScratch ploc;
    *startOver = false;
    if ((rc = triangleRecords(r, refit)) != PTX_OK || (rc = leafReferences(r, refit, keepState, &refs)) != PTX_OK)
        return rc;
    const uint32_t slotCap = std::max(refs.n, nTri); // triangle slots: split copies, or every triangle once when references pair them
    if (!refit && ((rc = referenceBuffers(r, refs.n, slotCap, ploc)) != PTX_OK || (rc = sortReferences(r, refs)) != PTX_OK))
        return rc;
    // triangle slots in the tree: the references', plus the second triangle of every pair (pairs are live: all in the tree)
    const uint32_t nv = B.treeTris, pairLeaves = B.pairRefs ? nTri - refs.n : 0u, slots = nv + pairLeaves;
    r->accel.tree.slots = slots;
    r->stats.bvhNodes = r->accel.tree.nodeCount = nv > 1 ? nv - 1 : (nv ? 1 : 0);
    r->stats.treeReferences = r->accel.tree.references = slots;
    r->stats.treeTriangles = nTri - (refs.n - nv); // a zero-area triangle has exactly one reference, and they are the ones left out
    if (r->env.verbose && !refit && B.pairRefs)
        std::fprintf(stderr, "[ptx] pair leaves: %u (%u of %u tree triangles paired)\n", pairLeaves, 2 * pairLeaves, slots);
    if (nv == 1)
        k_single_leaf_root<<<1, 1, 0, r->stream>>>(B.vals0.p, refs.lo, refs.hi, B.triTmp.p, r->accel.tree.nodes.p, r->accel.tree.tris.p, r->scene.pairs.p, r->scene.vertices.p,
                                                   r->scene.indices.p, r->accel.tree.shadeTris.p, refs.tri, refs.pair);
    else if (nv > 1)
    {
        if (refit)
            rc = bottomUpPass(r, refs, nv, false, false);
        else if ((rc = binaryTopology(r, refs, nv, ploc)) == PTX_OK && r->accel.params.reinsertPasses && !r->accel.reinsertBroken && nv > 3)
            rc = reinsertionPasses(r, refs, nv, r->accel.params.reinsertPasses, startOver);
        if (rc != PTX_OK || *startOver)
            return rc;
        // (PLOC computes its boxes itself: in a full build no pass before may have asked for the level lists yet)
        if (r->accel.params.collapse && (rc = bottomUpPass(r, refs, nv, true, !refit && !B.levelsValid)) != PTX_OK)
            return rc;
        k_emit<<<(nv + 255) / 256, 256, 0, r->stream>>>((int)nv, B.vals0.p, refs.lo, refs.hi, B.children.p, B.nodeLo.p, B.nodeHi.p, B.triTmp.p,
                                                       B.rawNodes.p, r->accel.tree.tris.p, r->scene.pairs.p, r->scene.vertices.p, r->scene.indices.p, r->accel.tree.shadeTris.p,
                                                       r->accel.params.collapse ? B.collapseDecide.p : nullptr, refs.tri, B.pairRefs ? B.slotOf.p : nullptr, refs.pair);
        if ((rc = relayoutNodes(r, refs.n, nv)) != PTX_OK)
            return rc;
    }
    if (r->scene.anyNonOpaque && nv) // the any-hit records of the slots k_emit has just written
    {
        HIP_TRY(r, r->accel.tree.alphaTris.alloc(slotCap));
        k_alpha_tris<<<(slots + 255) / 256, 256, 0, r->stream>>>(slots, r->accel.tree.tris.p, r->accel.tree.shadeTris.p, makeSceneView(r), r->scene.alphaTexOf.p, r->scene.alphaTex.p, r->accel.tree.alphaTris.p);
    }
    uint32_t revived = 0;
    if (refit)
        HIP_TRY(r, hipMemcpyAsync(&revived, &B.sceneBounds.p[7], sizeof(revived), hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(r, hipEventRecord(r->launch.evB.get(), r->stream));
    HIP_TRY(r, hipStreamSynchronize(r->stream));
    HIP_TRY(r, hipGetLastError());
    *startOver = revived != 0; // a triangle the last full build left out has an area now: it is not in the kept topology
    return PTX_OK;
}

// Full build (refit = false) or refit of the tree over the uploaded triangles.  keepState leaves the temporaries allocated
// for later refits; a static scene frees them.
static int buildAccel(PtxRenderer *r, bool refit, bool keepState)
{
    HIP_TRY(r, hipSetDevice(r->device));
    if (r->scene.triCount == 0)
    {
        if (!refit)
        {
            HIP_TRY(r, r->accel.tree.nodes.alloc(1)); HIP_TRY(r, r->accel.tree.tris.alloc(1)); HIP_TRY(r, r->accel.tree.shadeTris.alloc(1));
        }
        r->accel.ready = true;
        r->accel.tree.slots = 0;
        r->stats.bvhNodes = r->accel.tree.nodeCount = 0;
        r->stats.treeTriangles = r->stats.treeReferences = r->accel.tree.references = 0;
        r->stats.lastBuildMs = 0.0;
        return PTX_OK;
    }
    bool startOver = false;
    int rc = buildOnce(r, refit, keepState, &startOver);
    while (rc == PTX_OK && startOver) // (twice at most: a refit, a full build, a full build without reinsertion)
        rc = buildOnce(r, false, keepState, &startOver);
    if (rc == PTX_OK && keepState)
        r->accel.build.valid = true;
    else
        r->accel.build = BuildState(); // (a failed build leaves no state behind, a static scene frees its temporaries)
    if (rc != PTX_OK)
        return rc;
    float ms = 0.0f;
    (void)hipEventElapsedTime(&ms, r->launch.evA.get(), r->launch.evB.get());
    r->stats.lastBuildMs = ms;
    r->accel.ready = true;
    return PTX_OK;
}

// The price of the tree just built on the sampled segments (k_sample_tree_cost): mean visits + tests per ray, the tail, and
// the figure the candidates are compared by.  The tail term: a persistent traversal launch ends with its longest ray, and in the
// thin launches of late bounces and of small tile shards that ray IS the launch -- a tree that saves 1 % on the mean and grows
// its longest walks by a third is not cheaper.
struct TreeCost
{
    double mean = 0.0;   // visits + tests per ray, without the top 0.1 % of the rays (robust against the odd ray that skims a surface)
    uint32_t p999 = 0;   // 99.9th percentile
    uint32_t worst = 0;
    double figure() const { return mean + kTreeTailWeight * (double)p999; }
    static constexpr double kTreeTailWeight = 0.02; // a p99.9 five times the mean adds 10 % to the figure
};
constexpr uint32_t kTreeSampleRays = 65536;

static int sampleTreeCost(PtxRenderer *r, DevBuf<float4> &segments, bool drawSegments, TreeCost *cost)
{
    DevBuf<uint32_t> d;
    HIP_TRY(r, d.alloc(kTreeSampleRays));
    HIP_TRY(r, segments.alloc(2 * (size_t)kTreeSampleRays));
    const TraceScene sc = makeTraceScene(r);
    if (drawSegments)
        k_sample_segments<<<kTreeSampleRays / kBlock, kBlock, 0, r->stream>>>(sc, kTreeSampleRays, segments.p);
    if (r->scene.anyNonOpaque)
        k_sample_tree_cost<true><<<kTreeSampleRays / kBlock, kBlock, 0, r->stream>>>(sc, segments.p, kTreeSampleRays, r->launch.spill.p, d.p);
    else
        k_sample_tree_cost<false><<<kTreeSampleRays / kBlock, kBlock, 0, r->stream>>>(sc, segments.p, kTreeSampleRays, r->launch.spill.p, d.p);
    std::vector<uint32_t> h(kTreeSampleRays);
    HIP_TRY(r, hipMemcpyAsync(h.data(), d.p, kTreeSampleRays * sizeof(uint32_t), hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(r, hipStreamSynchronize(r->stream));
    HIP_TRY(r, hipGetLastError());
    std::sort(h.begin(), h.end());
    const uint32_t kept = kTreeSampleRays - kTreeSampleRays / 1000;
    unsigned long long sum = 0;
    for (uint32_t k = 0; k < kept; k++)
        sum += h[k];
    cost->mean = (double)sum / kept;
    cost->p999 = h[kept - 1];
    cost->worst = h.back();
    return PTX_OK;
}

// What buildBestTree varies from tree to tree, and `given` with one candidate's values in place
struct TreeCandidate { uint32_t radius; float shape; bool cubic; };
static TreeParams withCandidate(TreeParams t, const TreeCandidate &c) { t.plocRadius = c.radius; t.plocShape = c.shape; t.mortonCubic = c.cubic; return t; }

static int buildBestTree(PtxRenderer *r)
{
    if (r && r->link.owner)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "ptx_build_accel: this renderer shares another renderer's scene (ptx_share_scene)");
    if (!r || !r->link.ready)
        return fail(r, PTX_ERROR_NOT_READY, "ptx_build_accel: no scene uploaded");
    quiesceSharers(r);
    r->link.epoch++; // schedules learnt on the old tree's scene are not this one's (ptx_scene_upload without a build in between cannot render)
    // Which tree?  Build a few candidates, price each on the same sampled surface-to-surface segments, keep the cheapest (its
    // buffers are swapped aside while the others are built; lastBuildMs is the time of everything).  Parameters given in the
    // environment, the Karras builder and small scenes skip the comparison; the per-frame rebuilds of an animation use the
    // parameters chosen here.
    // (round 4, on the cosine-ray sampler, twelve settings tried per stand-in: these seven hold every scene's best or come within
    // 0.3 % of it -- chess_like (64, 0.25), atrium_like (4, 0.25), street_like (8, 1, cubic), temple_like (16, 0.25); the spread
    // between best and worst setting of a scene is 5-10 %)
    static const TreeCandidate kTreeCandidates[] = { { 8u, 0.0f, false }, { 16u, 0.0f, false }, { 16u, 0.25f, false }, { 32u, 1.0f, false }, { 8u, 1.0f, true },
                                                     { 64u, 0.25f, false }, { 4u, 0.25f, false } };
    constexpr uint32_t kCandidates = sizeof(kTreeCandidates) / sizeof(kTreeCandidates[0]);
    if (!r->accel.usePloc || r->env.plocFixed || r->scene.triCount < 4096u)
    {
        // ONE tree: it gets the full number of reinsertion passes at once
        const TreeParams keep = r->accel.params;
        r->accel.params.reinsertPasses = std::max(keep.reinsertPasses, keep.reinsertFinal);
        const int rc = buildAccel(r, false, false);
        r->accel.params = keep;
        return rc;
    }
    AccelState::Tree bestTree; // buffers and size together (leaf slots: with pre-splitting the candidates can differ -- cubic cells move the cut planes)
    DevBuf<float4> segments;
    TreeCost cost[kCandidates];
    double totalMs = 0.0;
    uint32_t best = 0, built = 0;
    const TreeParams given = r->accel.params; // what the candidates do not vary (the collapse)
    // While candidates are built the renderer's tree is whichever was built last and the best one sits in the local
    // above: nothing may render (or borrow the scene) until the final swap.  A candidate that fails (out of memory, a device
    // error) does not take the scene down with it when an earlier one succeeded: that tree, its parameters and its node count
    // are put back and the build succeeds with it.
    r->accel.ready = false;
    for (uint32_t k = 0; k < kCandidates; k++)
    {
        r->accel.params = withCandidate(given, kTreeCandidates[k]);
        int rc = buildAccel(r, false, false);
        totalMs += r->stats.lastBuildMs;
        if (rc != PTX_OK || (rc = sampleTreeCost(r, segments, k == 0, &cost[k])) != PTX_OK)
        {
            r->accel.ready = false;
            if (k == 0)
                return rc; // no tree at all: the error stands (ptx_last_error has the text)
            if (r->env.verbose)
                std::fprintf(stderr, "[ptx] tree candidate %u failed (%s): keeping candidate %u\n", k, r->error.c_str(), best);
            break;
        }
        built = k + 1;
        if (k == 0 || cost[k].figure() < cost[best].figure())
        {
            best = k;
            r->accel.tree.swap(bestTree); // the renderer's tree is now the previous best (or nothing): the next candidate is built over it
        }
    }
    // The winner once more, with the full number of reinsertion passes (the candidates had a few: the ranking is the same with 2
    // as with 64, the cost keeps falling for dozens of passes).  Built over the renderer's buffers -- they hold a loser --, priced
    // on the same rays, and kept only if it is no worse; if it fails, the candidate stands.
    TreeCost finalCost;
    bool haveFinal = false;
    if (given.reinsertFinal > given.reinsertPasses && built > 0)
    {
        r->accel.params = withCandidate(given, kTreeCandidates[best]);
        r->accel.params.reinsertPasses = given.reinsertFinal;
        int rc = buildAccel(r, false, false);
        totalMs += r->stats.lastBuildMs;
        if (rc == PTX_OK && sampleTreeCost(r, segments, false, &finalCost) == PTX_OK && finalCost.figure() <= cost[best].figure())
            haveFinal = true;
        else if (r->env.verbose)
            std::fprintf(stderr, "[ptx] the fully re-optimised tree was not kept (%s)\n", rc == PTX_OK ? "no cheaper" : r->error.c_str());
        r->accel.ready = false;
    }
    if (!haveFinal)
        r->accel.tree.swap(bestTree);
    r->stats.bvhNodes = r->accel.tree.nodeCount; // the statistics are those of the tree in use
    r->stats.treeReferences = r->accel.tree.references;
    r->accel.params = withCandidate(given, kTreeCandidates[best]);
    r->stats.lastBuildMs = totalMs;
    r->accel.ready = true;
    if (r->env.verbose)
    {
        std::fprintf(stderr, "[ptx] tree cost on %u sampled rays, mean (lowest 99.9 %%) / p99.9 / max visits + tests per ray:", kTreeSampleRays);
        for (uint32_t k = 0; k < built; k++)
            std::fprintf(stderr, " (radius %u, shape %.2f%s) %.2f / %u / %u%s", kTreeCandidates[k].radius, kTreeCandidates[k].shape,
                         kTreeCandidates[k].cubic ? ", cubic cells" : "", cost[k].mean, cost[k].p999, cost[k].worst, k == best ? " <- kept" : "");
        if (haveFinal)
            std::fprintf(stderr, "; with %u reinsertion passes %.2f / %u / %u", given.reinsertFinal, finalCost.mean, finalCost.p999, finalCost.worst);
        std::fprintf(stderr, "; collapse %s, %u reinsertion passes per candidate; %.1f ms\n", given.collapse ? "cost-driven" : "greedy", given.reinsertPasses, totalMs);
    }
    return PTX_OK;
}
