"""MI355X-native Animatable Gaussians.  The modules are imported by name (``from animatablegaussians_amd import losses``); the two
loader-facing functions of ``targets``, the template stage's ``TemplateField`` with ``eikonal_loss`` and its renderer (``render``,
``render_normals``, ``near_far_smpl``, ``sample_pts_on_rays``, ``composite`` and, for training, ``composite_backward``, ``laplace_density``,
``render_train``, ``training_loss`` of ``template_render``, ``TemplateFieldModule`` of ``template_train``) and the hand fusion (``HandField``,
``hand_meshes``, ``fuse_hands``, ``hand_fields_from_checkpoint`` of ``hand_fusion``) and the ray selection (``get_rays``, ``get_near_far``,
``bound_mask``, ``candidates``, ``sample_randomly``, ``sample_patches``, ``image_rays``, ``render_image`` of ``ray_select``) are also reachable from the package,
resolved on first use so that importing the package stays free of side effects."""

__all__ = ["prepare_targets", "boundary_mask", "TemplateField", "eikonal_loss", "render", "render_normals", "near_far_smpl",
           "sample_pts_on_rays", "composite", "composite_backward", "laplace_density", "render_train", "training_loss", "TemplateFieldModule", "HandField", "hand_meshes", "fuse_hands", "hand_fields_from_checkpoint",
           "get_rays", "get_near_far", "bound_mask", "candidates", "sample_randomly", "sample_patches", "image_rays", "render_image"]

_HOME = {"prepare_targets": "targets", "boundary_mask": "targets", "TemplateField": "template_field", "eikonal_loss": "template_field",
         "render": "template_render", "render_normals": "template_render",
         "near_far_smpl": "template_render", "sample_pts_on_rays": "template_render", "composite": "template_render",
         "composite_backward": "template_render", "laplace_density": "template_render", "render_train": "template_render",
         "training_loss": "template_render", "TemplateFieldModule": "template_train",
         "HandField": "hand_fusion", "hand_meshes": "hand_fusion", "fuse_hands": "hand_fusion", "hand_fields_from_checkpoint": "hand_fusion",
         "get_rays": "ray_select", "get_near_far": "ray_select", "bound_mask": "ray_select", "candidates": "ray_select",
         "sample_randomly": "ray_select", "sample_patches": "ray_select", "image_rays": "ray_select", "render_image": "ray_select"}


def __getattr__(name):
    if name in _HOME:
        import importlib
        return getattr(importlib.import_module("." + _HOME[name], __name__), name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
