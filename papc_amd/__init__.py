"""papc_amd -- the MI355X (gfx950) hot path of AgentMaker/PAPC behind the reference's op signatures.

Public surface mirrors the reference:
  papc_amd.functional  <- PAPC/models/layers/pointnet2_basic_layers.py free functions
  papc_amd.layers      <- PointNetSetAbstraction(.Msg)
  papc_amd.pillars     <- PFNLayer / PillarFeatureNet (pointpillars/models/bones/pillars.py)
  papc_amd.models      <- PointNet2_SSG_Clas / PointNet2_MSG_Clas / PointNet_Basic_Clas / PointNet_Clas (T-Net PointNet),
                          PointNet2_SSG_Seg / PointNet2_MSG_Seg / PointNet_Seg / PointNet_Basic_Seg, KDNet, KDUNet, VoxNet
  papc_amd.transform   <- the T-Net PointNet's per-cloud transform x . T[b] and its T-Net FC blocks
  papc_amd.cloudconcat <- relu(bn(conv(concat([point, tile(global)])))) without the tile: the autograd node and BatchNorm sequence of both
                          concat-conv kernel families
  papc_amd.segment     <- the PointNet segmenters' first seg_net layer on it (the Cp = 64 family)
  papc_amd.vfe         <- the VFE models' wide concat layers on it (the K-looped family)
  papc_amd.kdnet       <- one KD-Net level (conv, ReLU, kd-tree select, pair max) computing only the selected third of the conv, and the KDUNet
                          down level (the same behind a BatchNorm whose statistics come from the input rows' moments)
  papc_amd.voxnet      <- the VoxNet backbone (two 3-D convs as implicit GEMMs, the norm on load, the pool in registers), the head's LeakyReLU +
                          dropout and the occupancy grid of a cloud
  papc_amd.detloss     <- the training branch of PointPillars.forward (detectors/pointpillars.py:150-213): prepare_loss_weights, create_loss,
                          add_sin_difference, _get_pos_neg_loss, get_direction_target and pointpillars_loss, the whole detection loss with its
                          three gradients as one autograd node
  papc_amd.detect      <- PointPillars.predict (detectors/pointpillars.py:218-398) and second_box_decode: score, top-k, box decode and NMS for a
                          whole batch as one launch sequence, counts on the device
  papc_amd.targets     <- the target half of prep_pointcloud (data/preprocess.py:251-302): the anchor generators, TargetAssigner, the occupied-area
                          anchor mask and assign() (create_target_np on the nearest-BEV IoU, second_box_encode) for a whole batch on the device
  papc_amd.rpn         <- RPN (pointpillars/models/bones/rpn.py): the dense 2-D backbone as implicit-GEMM 3x3 convolutions and kernel = stride
                          deconvolutions with the norm and ReLU applied on load, one autograd node from the canvas to the activated concat rows,
                          the three heads one fused row GEMM
  papc_amd.detector    <- PointPillars (detectors/pointpillars.py): PillarFeatureNet -> PointPillarsScatter -> RPN -> the loss or predict()
  papc_amd.datasets    <- PAPC/datasets loaders: PNClasDataLoader / PNSegDataLoader / KDClasDataLoader / KDSegDataLoader / VoxDataLoader
The compute lives in libpapc_hip.so (hand-written HIP, C ABI in include/papc_hip.h).
"""
__version__ = "0.1.0"
