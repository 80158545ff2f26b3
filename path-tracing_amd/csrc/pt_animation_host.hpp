// pt_animation_host.hpp -- ptx_track_motion and ptx_update_animation: the pose snapshot of the motion guides, the new instance and
// bone transforms, k_skin, and the refit or rebuild of the tree behind them.  Included by pt_runtime.hpp after pt_bvh_host.hpp (it
// calls buildAccel); the state is SceneData's animation members and SceneData::PoseTracking.
#pragma once

// Does the linear part of a mat3x4 have a negative determinant (an instance that mirrors its model)?
static bool transformMirrors(const float *m)
{
    const double det = (double)m[0] * ((double)m[5] * m[10] - (double)m[6] * m[9]) - (double)m[1] * ((double)m[4] * m[10] - (double)m[6] * m[8]) +
                       (double)m[2] * ((double)m[4] * m[9] - (double)m[5] * m[8]);
    return det < 0.0;
}

// ptx_track_motion: whether ptx_update_animation keeps the pose it replaces (snapshotPose).  Owner only, like the update itself.
static int trackMotion(PtxRenderer *r, int enable)
{
    if (!r)
        return PTX_ERROR_INVALID_ARGUMENT;
    if (r->link.owner)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "ptx_track_motion: this renderer shares another renderer's scene (ptx_share_scene)");
    if (!r->link.ready)
        return fail(r, PTX_ERROR_NOT_READY, "ptx_track_motion: no scene uploaded");
    SceneData::PoseTracking &pose = r->scene.pose;
    if (!enable && pose.enabled)
    {
        // a guide pass in flight may still read the snapshot
        HIP_TRY(r, hipSetDevice(r->device));
        quiesceSharers(r);
        HIP_TRY(r, hipStreamSynchronize(r->stream));
        pose.release();
    }
    pose.enabled = enable != 0;
    return PTX_OK;
}

// The first step of ptx_update_animation behind its checks: with tracking on the pose about to be replaced is kept -- the DevPair
// table and the skinned part of the vertex buffer, device to device on the render stream ahead of the uploads and k_skin.  With
// tracking off nothing is enqueued.  The snapshot counts, and the pose serial moves on, only once the update has succeeded
// (updateAnimation): a failed one leaves no snapshot, and the serial where it was.
static int snapshotPose(PtxRenderer *r)
{
    SceneData &sc = r->scene;
    sc.pose.snapshotValid = false;
    if (sc.pose.enabled)
    {
        HIP_TRY(r, sc.pose.prevPairs.alloc(sc.pairCount));
        HIP_TRY(r, sc.pose.prevSkinned.alloc(sc.skinnedCount));
        if (sc.pairCount)
            HIP_TRY(r, hipMemcpyAsync(sc.pose.prevPairs.p, sc.pairs.p, (size_t)sc.pairCount * sizeof(DevPair), hipMemcpyDeviceToDevice, r->stream));
        if (sc.skinnedCount)
            HIP_TRY(r, hipMemcpyAsync(sc.pose.prevSkinned.p, sc.vertices.p + sc.staticVertexCount, (size_t)sc.skinnedCount * sizeof(PtxVertex),
                                      hipMemcpyDeviceToDevice, r->stream));
    }
    return PTX_OK;
}

static int applyAnimation(PtxRenderer *r, const PtxTransform *instanceTransforms, const PtxTransform *boneTransforms, uint32_t boneCount, uint32_t accelUpdate);

// Renderer.cpp:1750-1754 (+ RecordSkinningCommands :854-890, AccelerationStructure::Update :48-57)
static int updateAnimation(PtxRenderer *r, const PtxTransform *instanceTransforms, uint32_t instanceCount, const PtxTransform *boneTransforms, uint32_t boneCount, uint32_t accelUpdate)
{
    if (!r || accelUpdate > PTX_ACCEL_REBUILD)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "ptx_update_animation: bad argument");
    if (r->link.owner)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "ptx_update_animation: this renderer shares another renderer's scene (ptx_share_scene)");
    if (!r->link.ready)
        return fail(r, PTX_ERROR_NOT_READY, "ptx_update_animation: no scene uploaded");
    quiesceSharers(r);
    if (instanceTransforms && instanceCount != r->scene.instanceCount)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "ptx_update_animation: %u instance transforms for a scene of %u instances", instanceCount,
                    r->scene.instanceCount);
    HIP_TRY(r, hipSetDevice(r->device));
    if (const int rc = snapshotPose(r))
        return rc;
    const int rc = applyAnimation(r, instanceTransforms, boneTransforms, boneCount, accelUpdate);
    if (rc == PTX_OK) // accepted: the serial moves on, and what snapshotPose kept is the pose of the serial before
    {
        r->scene.pose.serial++;
        r->scene.pose.snapshotValid = r->scene.pose.enabled;
    }
    return rc;
}

// the update itself, behind ptx_update_animation's checks and the snapshot
static int applyAnimation(PtxRenderer *r, const PtxTransform *instanceTransforms, const PtxTransform *boneTransforms, uint32_t boneCount, uint32_t accelUpdate)
{
    if (instanceTransforms)
    {
        for (size_t p = 0; p < r->scene.hostPairs.size(); p++)
        {
            DevPair &pr = r->scene.hostPairs[p];
            composeTransform(instanceTransforms[r->scene.pairInstance[p]].m, r->scene.pairMeshTransform[p].m, pr.M);
            inverseLinear(pr.M, pr.Rinv);
            r->scene.hostDebugPairs[p].flags = transformMirrors(instanceTransforms[r->scene.pairInstance[p]].m) ? kDebugPairMirrored : 0u;
        }
        if (!r->scene.hostPairs.empty())
        {
            HIP_TRY(r, hipMemcpyAsync(r->scene.pairs.p, r->scene.hostPairs.data(), r->scene.hostPairs.size() * sizeof(DevPair), hipMemcpyHostToDevice, r->stream));
            HIP_TRY(r, hipMemcpyAsync(r->scene.debugPairs.p, r->scene.hostDebugPairs.data(), r->scene.hostDebugPairs.size() * sizeof(DebugPair), hipMemcpyHostToDevice, r->stream));
        }
    }
    if (boneTransforms && r->scene.skinnedCount)
    {
        if (boneCount > r->scene.bones.n)
            HIP_TRY(r, r->scene.bones.alloc(boneCount));
        r->scene.boneCount = boneCount;
        if (boneCount)
            HIP_TRY(r, hipMemcpyAsync(r->scene.bones.p, boneTransforms, (size_t)boneCount * sizeof(PtxTransform), hipMemcpyHostToDevice, r->stream));
        k_skin<<<(r->scene.skinnedCount + 255) / 256, 256, 0, r->stream>>>(r->scene.animatedVertices.p, r->scene.skinSource.p, r->scene.skinnedCount, r->scene.bones.p, boneCount,
                                                                  r->scene.vertices.p + r->scene.staticVertexCount);
    }
    HIP_TRY(r, hipStreamSynchronize(r->stream)); // the caller's arrays may go away
    const bool refit = accelUpdate == PTX_ACCEL_REFIT && r->accel.build.valid && r->accel.ready;
    return buildAccel(r, refit, true);
}
