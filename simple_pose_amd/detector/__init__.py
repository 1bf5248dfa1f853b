"""YOLOv5 person detector (the reference's detector/ package): parameter holders under the reference's state_dict keys, lowered onto the
HIP library as one fp32 program per letterboxed shape (simple_pose_amd.engine.yolov5_program) plus the batched YOLO NMS (csrc/detect.hip)."""
