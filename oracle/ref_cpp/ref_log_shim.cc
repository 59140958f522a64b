// TEST INFRASTRUCTURE ONLY -- stand-in for the reference's cpp/fury/util/logging.cc, which needs
// abseil (not a dependency of this project).  Defines exactly the five symbols that
// fury/util/logging.h declares and the row code links against: GetCallTrace, the FuryLog
// constructor and destructor, IsLevelEnabled and GetLogLevel.  A FATAL log (a failed FURY_CHECK)
// aborts, as the reference's does; nothing below WARNING is printed.
#include <cstdlib>
#include <iostream>
#include <string>

#include "fury/util/logging.h"

namespace fury {

std::string GetCallTrace() { return std::string(); }

FuryLog::FuryLog(const char *file_name, int line_number, FuryLogLevel severity)
    : severity_(severity) {
  Stream() << file_name << ":" << line_number << ": ";
}

FuryLog::~FuryLog() {
  Stream() << std::endl;
  if (severity_ == FuryLogLevel::FURY_FATAL) {
    std::abort();
  }
}

bool FuryLog::IsLevelEnabled(FuryLogLevel log_level) { return log_level >= GetLogLevel(); }

FuryLogLevel FuryLog::GetLogLevel() { return FuryLogLevel::FURY_WARNING; }

} // namespace fury
