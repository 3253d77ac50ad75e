"""The part of the hand that every face of the rendered mesh belongs to: pure integer work on the host, done once per
player, numpy and no device.  A label is 1 + the index of the skinning joint that moves the surface most; 0 is the background."""
import numpy as np

MANO_PARTS = ("wrist", "index1", "index2", "index3", "middle1", "middle2", "middle3", "pinky1", "pinky2", "pinky3", "ring1", "ring2", "ring3",
              "thumb1", "thumb2", "thumb3")
_FINGERS = tuple(f"{f}{k}" for f in ("index", "middle", "pinky", "ring", "thumb") for k in (1, 2, 3))
# the 55 joints of the SMPL-X tree in the model's order
SMPLX_PARTS = (("pelvis", "left_hip", "right_hip", "spine1", "left_knee", "right_knee", "spine2", "left_ankle", "right_ankle", "spine3", "left_foot",
                "right_foot", "neck", "left_collar", "right_collar", "head", "left_shoulder", "right_shoulder", "left_elbow", "right_elbow",
                "left_wrist", "right_wrist", "jaw", "left_eye", "right_eye") + tuple("left_" + n for n in _FINGERS) +
               tuple("right_" + n for n in _FINGERS))


def vertex_part_labels(weights):
    """skinning weights (V0, NJ) -> (V0,) uint8: 1 + the joint with the largest weight, ties to the lower joint"""
    w = np.asarray(weights)
    if w.ndim != 2 or w.shape[0] < 1 or not 1 <= w.shape[1] <= 255:
        raise ValueError(f"weights must be (V0, NJ) with NJ in 1..255, got {tuple(w.shape)}")
    return (1 + np.argmax(w, axis=1)).astype(np.uint8)          # (argmax: the first of equal weights)


def subdivided_vertex_part_labels(weights, edges0):
    """The part of every VERTEX of the once-subdivided mesh: weights (V0, NJ), edges0 (E0, 2) the base edges in the order of their
    midpoints (topology.subdivide_topology) -> (V0 + E0,) uint8.  A base vertex by vertex_part_labels, the rule face_part_labels votes
    with; midpoint V0 + e by the same rule on the mean of its two ends' weights, which is how the subdivision skins it."""
    w, e = np.asarray(weights), np.asarray(edges0).reshape(-1, 2).astype(np.int64)
    base = vertex_part_labels(w)
    if e.shape[0] == 0:
        return base
    if e.min() < 0 or e.max() >= w.shape[0]:
        raise ValueError(f"edges0 must index the {w.shape[0]} base vertices")
    return np.concatenate([base, vertex_part_labels(0.5 * (w[e[:, 0]].astype(np.float64) + w[e[:, 1]].astype(np.float64)))])


def face_part_labels(weights, faces0, V0):
    """The part of every face of the once-subdivided mesh: weights (V0, NJ) skinning weights, faces0 (F0, 3) the base faces -> (4 F0,)
    uint8 in 1..NJ, in the face order [f0; f1; f2; f3] of topology.subdivide_topology.  A base vertex's part is 1 + the argmax of its
    weights (ties to the lower joint); corner sub-face i + k F0, k = 0, 1, 2, takes the part of corner k of base face i; the centre face
    i + 3 F0 takes the most frequent of the three, and corner 0's when all three differ."""
    w, f = np.asarray(weights), np.asarray(faces0)
    V0 = int(V0)
    if w.ndim != 2 or w.shape[0] != V0:
        raise ValueError(f"weights must be ({V0}, NJ), got {tuple(w.shape)}")
    if f.ndim != 2 or f.shape[1] != 3 or f.shape[0] < 1 or f.dtype.kind not in "iu" or f.min() < 0 or f.max() >= V0:
        raise ValueError(f"faces0 must be (F0, 3) integers in [0, {V0}), got {f.dtype} {tuple(f.shape)}")
    c = vertex_part_labels(w)[f.astype(np.int64)]               # (F0, 3): the corners' parts
    centre = np.where(c[:, 1] == c[:, 2], c[:, 1], c[:, 0])     # two or three equal: that one (1 == 2, else 0 is in the majority or all differ)
    return np.concatenate([c[:, 0], c[:, 1], c[:, 2], centre]).astype(np.uint8)


def joint_part_names(nj):
    """the names of the labels of a model with nj skinning joints, index = label: "background", then one per joint"""
    names = {len(MANO_PARTS): MANO_PARTS, len(SMPLX_PARTS): SMPLX_PARTS}.get(int(nj))
    return ["background"] + (list(names) if names is not None else [f"joint{j}" for j in range(int(nj))])


def part_names(hand_layer):
    """the names of the labels of `hand_layer`'s model, index = label: "background", then one per skinning joint (MANO: 16; the SMPL-X
    arm: the 55 joints of its tree, of which the faces carry those that own at least one vertex)"""
    return joint_part_names(np.asarray(hand_layer._model_np["weights"]).shape[1])
